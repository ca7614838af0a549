"""Timings of the rasterizer fragments (ops.rasterize_fragments): forward and backward (all three upstream
gradients) at 64 frames @256^2 of the bird template, K in {1, 8, 20}, with hipEvents around each call.

Bytes moved are computed from the shapes (what must cross memory at least: the four output planes written by the
forward; pix_to_face plus the three gradient planes read by the backward, its grad_verts written), and set against
the 6.3 TB/s copy rate measured on the MI355X.  Prints one line per case and a JSON line at the end.

    python tools/fragments_bench.py [--frames 64] [--img 256] [--iters 20] [--warmup 5] [--blur SIL]"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_TBS = 6.3   # measured device copy rate (TB/s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--img", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--K", type=str, default="1,8,20")
    ap.add_argument("--clip", action="store_true")
    args = ap.parse_args()
    from acfm_video_3d_reconstruction_amd import ops
    from acfm_video_3d_reconstruction_amd.synthetic import batch_verts, make_cams
    dev = torch.device("cuda:0")
    m = np.load(os.path.join(ROOT, "tests", "golden", "meshes.npz"))
    v_np, f_np = m["bird_v"], m["bird_f"]
    N, H = args.frames, args.img
    rng = np.random.default_rng(0)
    verts = torch.tensor(batch_verts(v_np, N, rng, 0.01), device=dev)
    cams = torch.tensor(make_cams(N, rng, extent=float(np.abs(v_np).max())), device=dev)
    faces = torch.from_numpy(np.ascontiguousarray(f_np)).to(dev)
    with torch.no_grad():
        ndc = (ops.project(verts, cams) * torch.tensor([-1.0, -1.0, 1.0], device=dev) +
               torch.tensor([0.0, 0.0, 2.732], device=dev)).contiguous()
    V, F = ndc.shape[1], faces.shape[0]
    blur = math.log(1.0 / 1e-4 - 1.0) * 1e-4
    rows = []
    for K in [int(k) for k in args.K.split(",")]:
        b = 0.0 if K == 1 else blur
        tv = ndc.clone().requires_grad_(True)
        gz = torch.randn(N, H, H, K, device=dev)
        gb = torch.randn(N, H, H, K, 3, device=dev)
        gd = torch.randn(N, H, H, K, device=dev)
        fwd_ms, bwd_ms = [], []
        for it in range(args.warmup + args.iters):
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record()
            p2f, zbuf, bary, dists = ops.rasterize_fragments(tv, faces, H, K, blur_radius=b,
                                                             clip_barycentric_coords=args.clip)
            e1.record()
            torch.autograd.backward([zbuf, bary, dists], [gz, gb, gd])
            e2.record()
            torch.cuda.synchronize()
            if it >= args.warmup:
                fwd_ms.append(e0.elapsed_time(e1))
                bwd_ms.append(e1.elapsed_time(e2))
            tv.grad = None
        P = N * H * H
        fwd_bytes = P * K * (8 + 4 + 12 + 4)
        bwd_bytes = P * K * (8 + 4 + 12 + 4) + N * V * 12
        fm, bm = float(np.median(fwd_ms)), float(np.median(bwd_ms))
        row = dict(K=K, blur=b, clip=bool(args.clip), fwd_us=1e3 * fm, bwd_us=1e3 * bm, fwd_bytes=fwd_bytes,
                   bwd_bytes=bwd_bytes, fwd_GBs=fwd_bytes / fm / 1e6, bwd_GBs=bwd_bytes / bm / 1e6,
                   fwd_bound_us=fwd_bytes / (COPY_TBS * 1e6), bwd_bound_us=bwd_bytes / (COPY_TBS * 1e6),
                   fwd_min_us=1e3 * min(fwd_ms), bwd_min_us=1e3 * min(bwd_ms))
        row["fwd_frac_of_copy"] = row["fwd_GBs"] / (COPY_TBS * 1e3)
        row["bwd_frac_of_copy"] = row["bwd_GBs"] / (COPY_TBS * 1e3)
        rows.append(row)
        print("K=%2d  fwd %8.1f us (%6.0f GB/s, %.2f of copy; bound %.0f us)   bwd %8.1f us (%6.0f GB/s, %.2f of copy; "
              "bound %.0f us)" % (K, row["fwd_us"], row["fwd_GBs"], row["fwd_frac_of_copy"], row["fwd_bound_us"],
                                  row["bwd_us"], row["bwd_GBs"], row["bwd_frac_of_copy"], row["bwd_bound_us"]))
        del p2f, zbuf, bary, dists, gz, gb, gd, tv
    print(json.dumps(dict(frames=N, img=H, mesh="bird", V=V, F=F, copy_TBs=COPY_TBS, rows=rows)))


if __name__ == "__main__":
    main()
