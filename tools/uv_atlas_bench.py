"""Timing of the texture head's tail (mesh_net.py:169-179), forward + backward, at the reference's size: B = 16 UV images
of 128 x 256, the symmetric level-3 sphere's sampler (F' = 656, S = 624, T = 6) -> atlases [16,1280,6,6,3] and back.
Two variants: ops.uv_atlas (HIP kernels, the table built once), and the same lines composed from torch ops on the GPU
(grid_sample, permute, tanh, cat and their autograd) -- an independent formulation, not the code under test.  Events
around every iteration, warm-up, median.
usage: python tools/uv_atlas_bench.py [--reps 100] [--batch 16]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
from acfm_video_3d_reconstruction_amd import ops, texture

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=100)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--batch", type=int, default=16)
a = ap.parse_args()
assert a.reps >= 50
d = torch.device("cuda:0")
torch.manual_seed(0)
fx = np.load(os.path.join(ROOT, "tests", "golden", "uv_atlas.npz"))
S = int(fx["num_sym_faces"])
Fp = int(fx["num_indept_faces"]) + S
T = 6
sampler = torch.tensor(texture.compute_uvsampler(fx["verts"], fx["faces"][:Fp], T), dtype=torch.float32, device=d)
Hu, Wu = texture.uv_image_size(Fp, T)
table = ops.uv_atlas_table(sampler, Hu, Wu)
x = torch.randn(a.batch, 3, Hu, Wu, device=d, requires_grad=True)
go = torch.randn(a.batch, Fp + S, T, T, 3, device=d)
grid = sampler.view(1, Fp, T * T, 2)


def hip_tail(img):
    return ops.uv_atlas(img, table, S)


def torch_tail(img):
    tex = torch.nn.functional.grid_sample(img, grid.repeat(img.shape[0], 1, 1, 1), align_corners=True)
    tex = tex.reshape(img.size(0), -1, Fp, T, T).permute(0, 2, 3, 4, 1)
    tex = (torch.tanh(tex) + 1) / 2
    return torch.cat([tex, tex[:, -S:]], 1)


def step(tail, backward=True):
    atlas = tail(x)
    return (atlas, torch.autograd.grad(atlas, x, go)[0]) if backward else (atlas, None)


def median_us(fn):
    for _ in range(a.warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)]
    for e0, e1 in ev:
        e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return sorted(e0.elapsed_time(e1) for e0, e1 in ev)[a.reps // 2] * 1e3


(a_hip, g_hip), (a_torch, g_torch) = step(hip_tail), step(torch_tail)
print("atlas: max |hip - torch| %.3e; gradient: max |hip - torch| %.3e of max|grad| %.3e"
      % (float((a_hip - a_torch).abs().max()), float((g_hip - g_torch).abs().max()), float(g_torch.abs().max())))
start = table.pix_start
print("table: %d entries, longest list %d, %d of %d pixels empty"
      % (table.n_entries, int((start[1:] - start[:-1]).max()), int((start[1:] == start[:-1]).sum()), Hu * Wu))
print("UV image -> atlas tail, B = %d, %d x %d, F' = %d, S = %d, T = %d, median of %d:" % (a.batch, Hu, Wu, Fp, S, T, a.reps))
for name, tail in (("HIP operator", hip_tail), ("torch ops", torch_tail)):
    print("  %-13s forward + backward %8.1f us   forward alone %8.1f us"
          % (name, median_us(lambda: step(tail)), median_us(lambda: step(tail, False))))
