"""Timing of the deformable convolution (csrc/acfm_dconv.hip) at MaskFlownet's five pyramid levels for a batch of 8
pairs (384 x 768 input): (C, H, W) = (196,6,12), (128,12,24), (96,24,48), (64,48,96), (32,96,192), Cin = Cout = C.
Three variants per level: ops.deform_conv2d with the 18-channel offset (the ninefold copy of the flow that
MaskFlownet.py:558-561 builds, made outside the timed call), the same with the 2-channel shared offset, and the torch
formulation flow_ops.deform_conv2d_torch on the same GPU tensors (nine grid_sample calls and an einsum: an independent
formulation, not the code under test; nothing in the package before this operator could be timed instead).  Events
around every iteration, warm-up, median.  Prints one JSON object.
usage: python tools/dconv_bench.py [--reps 100] [--warmup 10] [--batch 8] [--out FILE]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
from acfm_video_3d_reconstruction_amd import flow_ops, ops

LEVELS = ((196, 6, 12), (128, 12, 24), (96, 24, 48), (64, 48, 96), (32, 96, 192))

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=100)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--out", default=None)
a = ap.parse_args()
assert a.reps >= 50
assert torch.cuda.is_available(), "dconv_bench.py measures on the GPU only"
d = torch.device("cuda:0")
torch.manual_seed(0)


def median_us(fn):
    for _ in range(a.warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)]
    for e0, e1 in ev:
        e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return round(sorted(e0.elapsed_time(e1) for e0, e1 in ev)[a.reps // 2] * 1e3, 1)


levels = []
with torch.no_grad():
    for C, H, W in LEVELS:
        N = a.batch
        x = torch.randn(N, C, H, W, device=d)
        w = torch.randn(C, C, 3, 3, device=d) / (9 * C) ** 0.5
        b = torch.randn(C, device=d)
        flow = 2.0 * torch.randn(N, 2, H, W, device=d)
        off18 = flow.repeat(1, 9, 1, 1).contiguous()
        hip18 = lambda: ops.deform_conv2d(x, off18, w, b)
        hip2 = lambda: ops.deform_conv2d(x, flow, w, b, shared_offset=True)
        ref = lambda: flow_ops.deform_conv2d_torch(x, off18, w, b)
        r = ref()
        diff = float((hip18() - r).abs().max())
        assert torch.equal(hip18(), hip2())
        assert diff < 1e-3, diff
        levels.append({"C": C, "H": H, "W": W, "N": N,
                       "hip_offset18_us": median_us(hip18), "hip_shared_us": median_us(hip2),
                       "torch_composition_us": median_us(ref),
                       "max_abs_diff_hip_vs_torch": diff,
                       "gflop": round(2.0 * N * H * W * C * C * 9 / 1e9, 3)})
res = {"what": "deformable convolution forward, median of %d event-timed calls after %d warm-up calls, microseconds"
               % (a.reps, a.warmup),
       "device": torch.cuda.get_device_name(0), "levels": levels}
line = json.dumps(res)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
