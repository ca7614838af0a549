#!/usr/bin/env python3
"""In-graph cost of the three loss operators (ops.mask_losses, ops.tex_mse, ops.bds_loss_per_mesh) at the headline
shape: for each, a captured graph of --rep dependent calls is replayed, and the time per call printed (5 samples
of 20 replays).  Inside a replayed graph a launch costs what it costs in the real step, a zero-fill launch in
front of a kernel included, which a per-kernel event bracket does not show.

    python /path/to/tools/loss_graph_bench.py [--frames 64] [--img 256] [--points 800] [--verts 642] [--rep 20]

The package is imported from the CURRENT DIRECTORY, so the script measures the checkout it is run in: to measure
another commit, build that commit's checkout and run this file from its root.  (ACFM_LIB alone is not enough when
the two commits' Python layers call different entry points.)"""
import argparse
import os
import sys

import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--img", type=int, default=256)
    ap.add_argument("--points", type=int, default=800)
    ap.add_argument("--verts", type=int, default=642)
    ap.add_argument("--rep", type=int, default=20)
    a = ap.parse_args()
    sys.path.insert(0, os.getcwd())
    from acfm_video_3d_reconstruction_amd import ops
    d = torch.device("cuda:0")
    N, H, P, V = a.frames, a.img, a.points, a.verts
    g = torch.Generator().manual_seed(1)
    mask = torch.rand(N, H, H, generator=g).to(d)
    gt = (torch.rand(N, H, H, generator=g) > 0.5).float().to(d)
    edt = torch.rand(N, 1, H, H, generator=g).to(d)
    tex = torch.rand(N, 3, H, H, generator=g).to(d)
    img = torch.rand(N, 3, H, H, generator=g).to(d)
    xy = (torch.rand(N, V, 2, generator=g) * 2 - 1).to(d)
    bds = torch.cat([torch.rand(N, P, 2, generator=g) * 2 - 1, torch.ones(N, P, 1)], -1).to(d)
    vis = (torch.rand(N, V, generator=g) > 0.5).to(torch.uint8).to(d)
    fns = {"mask_losses": lambda: ops.mask_losses(mask, gt, edt),
           "tex_mse": lambda: ops.tex_mse(tex, img, gt),
           "bds_loss": lambda: ops.bds_loss_per_mesh(xy, bds, vis)}
    for name, fn in fns.items():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(graph):
            for _ in range(a.rep):
                fn()
        for _ in range(5):
            graph.replay()
        torch.cuda.synchronize()
        samples = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                graph.replay()
            e1.record()
            torch.cuda.synchronize()
            samples.append(e0.elapsed_time(e1) * 1e3 / (20 * a.rep))
        print("%-12s %s us/call (median %.2f)" % (name, " ".join("%.2f" % x for x in samples), sorted(samples)[2]))


if __name__ == "__main__":
    main()
