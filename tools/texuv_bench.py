"""Forward + backward of TexturesUV.sample_textures on the HIP kernel (ops.uv_texels) against PyTorch3D's composition of
torch operators (pytorch3d_shim...textures.uv_texels_composition: interpolate, K-fold expand of the map, flip,
grid_sample) on the same fragments: 64 bird meshes @256^2, K = 1 with blur 0 and K = 8 with the silhouette blur, maps
of 128x256 (the texture head's UV image) and 512x512.  Each path is timed eagerly (hipEvents, median of --iters; the
composition takes seconds per run and gets --comp-iters) and as a hipGraph replay, and its peak memory above the
inputs is printed.  Gradients go to the maps, verts_uvs and the barycentrics; the upstream gradient is exactly zero in
empty slots, as every shader sends it.

The backward of the kernel path is also timed alone -- with all three gradients, with the map's only and with the uv
side's only -- and its float-atomic bytes (4 bytes per non-zero contribution to grad_maps and grad_faces_verts_uvs,
counted on the host from the same inputs) are set against the first of these times; the figure is a lower bound of
the atomic rate, since the launch also reads its inputs, the call zero-fills and torch scatters the gathered
faces_verts_uvs gradient back to verts_uvs.

    python tools/texuv_bench.py [--frames 64] [--img 256] [--iters 10] [--warmup 3] [--comp-iters 2] [--comp-warmup 1]"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GUIDE_ATOMIC_TBS = 1.3   # chip-wide float-atomic rate of well-shaped adds (TB/s of added bytes)


def _timed(step, warmup, iters):
    ms = []
    for it in range(warmup + iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step()
        e1.record()
        torch.cuda.synchronize()
        if it >= warmup:
            ms.append(e0.elapsed_time(e1))
    return 1e3 * float(np.median(ms))


def _replayed(step, warmup, iters):
    from acfm_video_3d_reconstruction_amd import ops
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep = step()
    us = _timed(lambda: ops.graph_replay(graph), warmup, iters)
    del keep, graph
    return us


def _peak(step):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = step()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--img", type=int, default=256)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--comp-iters", type=int, default=2, help="timed runs of the composition (seconds each at K = 8)")
    ap.add_argument("--comp-warmup", type=int, default=1)
    args = ap.parse_args()
    from acfm_video_3d_reconstruction_amd import ops, texture
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.renderer import Fragments, TexturesUV
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.renderer.mesh.textures import uv_texels_composition
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
    uv0 = torch.tensor((texture.get_spherical_coords(v_np) + 1.0) / 2.0, dtype=torch.float32, device=dev)
    faces_uvs = faces[None].expand(N, -1, -1).contiguous()
    blur = math.log(1.0 / 1e-4 - 1.0) * 1e-4
    g = torch.Generator(device=dev).manual_seed(0)
    rows = []
    for K, b, clip in ((1, 0.0, True), (8, blur, False)):
        with torch.no_grad():
            p2f, zbuf, bary0, dists = ops.rasterize_fragments(ndc, faces, H, K, blur_radius=b,
                                                              clip_barycentric_coords=clip)
        live = p2f >= 0
        G = torch.randn(N, H, H, K, 3, device=dev, generator=g) * live[..., None]
        for Hm, Wm in ((128, 256), (512, 512)):
            maps = torch.rand(N, Hm, Wm, 3, device=dev, generator=g).requires_grad_(True)
            vu = uv0[None].expand(N, -1, -1).clone().requires_grad_(True)
            bary = bary0.clone().requires_grad_(True)
            tex = TexturesUV(maps=maps, faces_uvs=faces_uvs, verts_uvs=vu)
            fr = Fragments(p2f, zbuf, bary, dists)
            leaves = [maps, vu, bary]

            def kernel_fwd():
                return tex.sample_textures(fr)

            def comp_fwd():
                return uv_texels_composition(p2f, bary, tex.faces_verts_uvs_packed(), maps)

            def both(fwd):
                return lambda: torch.autograd.grad([fwd()], leaves, [G])

            with torch.no_grad():
                err = float((kernel_fwd() - comp_fwd()).abs().max())
            row = dict(K=K, blur=b, Hm=Hm, Wm=Wm, covered=float(live[..., 0].float().mean()), fwd_max_diff=err)
            for name, fwd, wu, it in (("kernel", kernel_fwd, args.warmup, args.iters),
                                      ("composition", comp_fwd, args.comp_warmup, args.comp_iters)):
                row[name + "_eager_us"] = _timed(both(fwd), wu, it)
                try:
                    row[name + "_replay_us"] = _replayed(both(fwd), wu, it)
                except RuntimeError as e:   # a path that cannot be captured is reported, not hidden
                    row[name + "_replay_us"] = float("nan")
                    row[name + "_replay_error"] = str(e).splitlines()[0][:200]
                row[name + "_peak_MB"] = _peak(both(fwd)) / 1e6
            # the kernel's backward alone (all three gradients, the map's only, the uv side's only), and the bytes
            # its float atomics add
            out = kernel_fwd()
            for key, lv in (("kernel_bwd_us", leaves), ("kernel_bwd_maps_only_us", [maps]),
                            ("kernel_bwd_uv_only_us", [vu, bary])):
                row[key] = _timed(lambda: torch.autograd.grad([out], lv, [G], retain_graph=True), args.warmup,
                                  args.iters)
            with torch.no_grad():
                fv = tex.faces_verts_uvs_packed()
                vals = fv[p2f.clamp(min=0)]
                uv = (bary[..., None] * vals).sum(dim=-2) * live[..., None]
                x, y = uv[..., 0] * (Wm - 1), uv[..., 1] * (Hm - 1)
                x, y = x.clamp(0, Wm - 1), y.clamp(0, Hm - 1)
                fx, fy = x - x.floor(), y - y.floor()
                wx = torch.stack([1 - fx, fx], -1) * torch.stack([x.floor() <= Wm - 1, x.floor() <= Wm - 2], -1)
                wy = torch.stack([1 - fy, fy], -1) * torch.stack([y.floor() <= Hm - 1, y.floor() <= Hm - 2], -1)
                w = wy[..., :, None] * wx[..., None, :]                                   # [N,H,H,K,2,2]
                n_maps = int(((w[..., None] * G[..., None, None, :]) != 0).sum())
                gsum = G.abs().sum(dim=-1) != 0
                n_fv = int((gsum & live).sum()) * 6                                        # an upper count
            row["atomic_MB"] = 4e-6 * (n_maps + n_fv)
            row["atomic_TBs_over_bwd"] = 4e-6 * (n_maps + n_fv) / row["kernel_bwd_us"]
            rows.append(row)
            print("K=%d map %dx%d: kernel %.0f us eager / %.0f replay, peak %.1f MB;  composition %.0f us eager / %.0f "
                  "replay, peak %.1f MB;  kernel backward %.0f us (maps only %.0f, uv side only %.0f) for %.1f MB of "
                  "float atomics = %.3f TB/s (guide: %.1f); forward max diff %.2g"
                  % (K, Hm, Wm, row["kernel_eager_us"], row["kernel_replay_us"], row["kernel_peak_MB"],
                     row["composition_eager_us"], row["composition_replay_us"], row["composition_peak_MB"],
                     row["kernel_bwd_us"], row["kernel_bwd_maps_only_us"], row["kernel_bwd_uv_only_us"],
                     row["atomic_MB"], row["atomic_TBs_over_bwd"], GUIDE_ATOMIC_TBS, err),
                  flush=True)
            del maps, vu, bary, tex, fr, out, vals, uv, w
        del p2f, zbuf, bary0, dists, G
    print(json.dumps(dict(frames=N, img=H, mesh="bird", guide_atomic_TBs=GUIDE_ATOMIC_TBS, rows=rows)))


if __name__ == "__main__":
    main()
