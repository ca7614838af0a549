"""Timings of the shaders over fragments (ops.sigmoid_alpha_blend, ops.atlas_softmax_blend, ops.softmax_rgb_blend),
forward and backward, at 64 frames @256^2 of the bird template, with hipEvents around each call (median of --iters).
The fragments are rasterized once per case and are not part of the timings.

Cases: the silhouette shader at K = 20 with the sigma blur; the fused atlas shader at K = 1 (blur 0, clipped, gamma
1e-4: the reference's texture render) and at K = 8 (blur, gamma 1e-2); the dense softmax blend at K = 8.  The least
bytes are computed from the shapes -- the fragment planes the blend must read (pix_to_face 8, dists 4, zbuf 4 bytes
per slot), the RGBA plane written (forward) or read (backward), the per-slot gradients written; colours / texels are
read only where a blend weight is non-zero and are not counted -- and set against the 6.3 TB/s copy rate.

    python tools/shader_bench.py [--frames 64] [--img 256] [--iters 20] [--warmup 5]"""
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
    args = ap.parse_args()
    from acfm_video_3d_reconstruction_amd import ops
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.renderer import BlendParams, Fragments
    from acfm_video_3d_reconstruction_amd.synthetic import batch_verts, make_cams
    dev = torch.device("cuda:0")
    m = np.load(os.path.join(ROOT, "tests", "golden", "meshes.npz"))
    v_np, f_np = m["bird_v"], m["bird_f"]
    N, H, R = args.frames, args.img, 6
    rng = np.random.default_rng(0)
    verts = torch.tensor(batch_verts(v_np, N, rng, 0.01), device=dev)
    cams = torch.tensor(make_cams(N, rng, extent=float(np.abs(v_np).max())), device=dev)
    faces = torch.from_numpy(np.ascontiguousarray(f_np)).to(dev)
    with torch.no_grad():
        ndc = (ops.project(verts, cams) * torch.tensor([-1.0, -1.0, 1.0], device=dev) +
               torch.tensor([0.0, 0.0, 2.732], device=dev)).contiguous()
    F = faces.shape[0]
    blur = math.log(1.0 / 1e-4 - 1.0) * 1e-4
    P = N * H * H
    g = torch.Generator(device=dev).manual_seed(0)
    atlas = torch.rand(N * F, R, R, 3, device=dev, generator=g)
    # name, K, blur, clip, kind, gamma
    cases = [("silhouette", 20, blur, False, "sigmoid", 1e-4), ("atlas K=1", 1, 0.0, True, "atlas", 1e-4),
             ("atlas K=8", 8, blur, False, "atlas", 1e-2), ("dense K=8", 8, blur, False, "dense", 1e-2)]
    rows = []
    for name, K, b, clip, kind, gamma in cases:
        with torch.no_grad():
            p2f, zbuf, bary, dists = ops.rasterize_fragments(ndc, faces, H, K, blur_radius=b,
                                                             clip_barycentric_coords=clip)
        d_, z_ = dists.clone().requires_grad_(True), zbuf.clone().requires_grad_(True)
        fr = Fragments(p2f, z_, bary, d_)
        bp = BlendParams(1e-4, gamma, 0.0)
        a_ = atlas.clone().requires_grad_(True)
        col = torch.rand(N, H, H, K, 3, device=dev, generator=g).requires_grad_(True) if kind == "dense" else None
        if kind == "sigmoid":
            run, leaves = (lambda: ops.sigmoid_alpha_blend(None, fr, bp)), [d_]
        elif kind == "atlas":
            run, leaves = (lambda: ops.atlas_softmax_blend(a_, fr, bp)), [a_, d_, z_]
        else:
            run, leaves = (lambda: ops.softmax_rgb_blend(col, fr, bp)), [col, d_, z_]
        G = torch.randn(N, H, H, 4, device=dev, generator=g)
        fwd_ms, bwd_ms = [], []
        for it in range(args.warmup + args.iters):
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record()
            out = run()
            e1.record()
            torch.autograd.grad([out], leaves, [G])
            e2.record()
            torch.cuda.synchronize()
            if it >= args.warmup:
                fwd_ms.append(e0.elapsed_time(e1))
                bwd_ms.append(e1.elapsed_time(e2))
        plane = 8 + 4 + (0 if kind == "sigmoid" else 4)           # pix_to_face, dists (, zbuf) per slot
        fwd_bytes = P * K * plane + P * 16
        bwd_bytes = P * K * plane + P * 16 + P * K * (4 if kind == "sigmoid" else 8)
        if kind == "atlas":
            bwd_bytes += atlas.numel() * 4                           # the atlas gradient, written once
        if kind == "dense":
            bwd_bytes += P * K * 12                                  # the dense colour gradient
        fm, bm = float(np.median(fwd_ms)), float(np.median(bwd_ms))
        row = dict(case=name, K=K, blur=b, clip=clip, gamma=gamma, fwd_us=1e3 * fm, bwd_us=1e3 * bm,
                   fwd_bytes=fwd_bytes, bwd_bytes=bwd_bytes, fwd_bound_us=fwd_bytes / (COPY_TBS * 1e6),
                   bwd_bound_us=bwd_bytes / (COPY_TBS * 1e6))
        row["fwd_frac_of_copy"] = row["fwd_bound_us"] / row["fwd_us"]
        row["bwd_frac_of_copy"] = row["bwd_bound_us"] / row["bwd_us"]
        rows.append(row)
        print("%-11s fwd %8.1f us (%.2f of copy; %.0f MB, bound %.0f us)   bwd %8.1f us (%.2f of copy; %.0f MB, "
              "bound %.0f us)" % (name, row["fwd_us"], row["fwd_frac_of_copy"], fwd_bytes / 1e6, row["fwd_bound_us"],
                                  row["bwd_us"], row["bwd_frac_of_copy"], bwd_bytes / 1e6, row["bwd_bound_us"]))
        del p2f, zbuf, bary, dists, d_, z_, fr, a_, col, out
    print(json.dumps(dict(frames=N, img=H, mesh="bird", F=F, R=R, copy_TBs=COPY_TBS, rows=rows)))


if __name__ == "__main__":
    main()
