"""Timing of the perceptual texture loss (perceptual.PerceptualTextureLoss over csrc/acfm_lpips.hip) against the literal
torch composition of the same definition (what lpips.LPIPS(spatial=True) and loss_utils.py:359-383 do, op by op), at
the reference's documented size: B = 8, G = 6, T = 2 -> Nr = 16 frames, N = 96 predictions, 256 x 256; once as one call
(N = 96) and once as the step's two calls (original + flipped, 192 predictions).  Forward + backward to img_pred.
AlexNet's weights are random (timing does not depend on them).  Three things are kept apart, each a median of event-
timed iterations after warm-up, milliseconds:
  conv      AlexNet on the predictions alone, forward + backward (torch / MIOpen; the same in both forms)
  tail      everything else on the prediction path, the convolutions cut out: the input chain, and on given feature
            stacks the layer distances, upsampling, mask and means, forward + backward -- ours vs the literal ops
  ref side  input chain + features of the reference images (+ the mask's weights, ours): the literal form runs them for
            all N repeated images, ours for the Nr distinct ones
and the totals of both forms.  Prints one JSON object.
usage: python tools/lpips_bench.py [--reps 20] [--warmup 3] [--frames 16] [--guesses 6] [--size 256] [--out FILE]"""
import argparse
import json
import os
import sys
import warnings

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
from acfm_video_3d_reconstruction_amd import ops, perceptual

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--frames", type=int, default=16)
ap.add_argument("--guesses", type=int, default=6)
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--out", default=None)
a = ap.parse_args()
assert torch.cuda.is_available(), "lpips_bench.py measures on the GPU only"
d = torch.device("cuda:0")
torch.manual_seed(0)
Nr, G, H = a.frames, a.guesses, a.size
N = Nr * G
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    feats = perceptual.AlexFeatures().to(d)
loss_fn = perceptual.PerceptualTextureLoss(feats)
SHIFT = torch.tensor(ops.LPIPS_SHIFT, device=d)[None, :, None, None]
SCALE = torch.tensor(ops.LPIPS_SCALE, device=d)[None, :, None, None]


def median_ms(fn):
    for _ in range(a.warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)]
    for e0, e1 in ev:
        e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return round(sorted(e0.elapsed_time(e1) for e0, e1 in ev)[a.reps // 2], 3)


def lit_input(img, m):
    return ((2 * (img * m) - 1) - SHIFT) / SCALE


def lit_norm(x):
    return x / (torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True)) + 1e-10)


def lit_tail(fa, fb, m):
    smap = sum(F.interpolate(((lit_norm(x) - lit_norm(y)) ** 2).sum(1, keepdim=True), size=(H, H), mode="bilinear",
                             align_corners=False) for x, y in zip(fa, fb))
    return (smap * m).mean(-2).mean(-1).squeeze(-1)


def literal(pred, img_rep, mask_rep):
    m = mask_rep[:, None]
    return lit_tail(feats(lit_input(pred, m)), feats(lit_input(img_rep, m)), m)


pred = torch.rand(N, 3, H, H, device=d, requires_grad=True)
imgs = [torch.rand(Nr, 3, H, H, device=d)]
masks = [(torch.rand(Nr, 1, H // 8, H // 8, device=d) > 0.4).float().repeat_interleave(8, 2).repeat_interleave(8, 3)[:, 0]
         .contiguous()]
imgs.append(imgs[0].flip(3).contiguous()); masks.append(masks[0].flip(2).contiguous())
imgs_rep = [t.repeat(G, 1, 1, 1) for t in imgs]
masks_rep = [t.repeat(G, 1, 1) for t in masks]


def total_ours(calls):
    def fn():
        loss = sum(loss_fn(pred, imgs[k], None, masks[k]) for k in range(calls))
        torch.autograd.grad(loss, pred)
    return fn


def total_literal(calls):
    def fn():
        loss = sum(literal(pred, imgs_rep[k], masks_rep[k]).mean() for k in range(calls))
        torch.autograd.grad(loss, pred)
    return fn


# the pieces, for one call of N predictions
x_in = torch.randn(N, 3, H, H, device=d, requires_grad=True)
with torch.no_grad():
    taps0 = feats(x_in)
    ref_rep = feats(lit_input(imgs_rep[0], masks_rep[0][:, None]))
g_taps = [torch.randn_like(t) for t in taps0]
g_x = torch.randn(N, 3, H, H, device=d)
leaf = [t.clone().requires_grad_(True) for t in taps0]
prepared = loss_fn.prepare(imgs[0], masks[0])


def conv():
    torch.autograd.grad(feats(x_in), x_in, g_taps)


def tail_ours():
    x = ops.lpips_input(pred, masks[0])
    torch.autograd.grad(x, pred, g_x)
    loss = ops.lpips_masked_mean(ops.lpips_layers(leaf, prepared.feats), prepared.M).mean()
    torch.autograd.grad(loss, leaf)


def tail_literal():
    m = masks_rep[0][:, None]
    x = lit_input(pred, m)
    torch.autograd.grad(x, pred, g_x)
    loss = lit_tail(leaf, ref_rep, m).mean()
    torch.autograd.grad(loss, leaf)


def ref_ours():
    loss_fn.prepare(imgs[0], masks[0])


def ref_literal():
    with torch.no_grad():
        feats(lit_input(imgs_rep[0], masks_rep[0][:, None]))


# the two forms agree before anything is timed
lo = loss_fn(pred, imgs[0], None, masks[0], reduce=False)
ll = literal(pred, imgs_rep[0], masks_rep[0])
diff = float((lo - ll).detach().abs().max())
assert diff <= 1e-4 * float(ll.detach().abs().max()), diff
res = {"what": "perceptual texture loss forward + backward, median of %d event-timed iterations after %d warm-up, ms"
               % (a.reps, a.warmup),
       "device": torch.cuda.get_device_name(0), "Nr": Nr, "N": N, "size": H,
       "max_abs_diff_ours_vs_literal": diff, "loss_max": float(ll.detach().abs().max()),
       "one_call": {"ours_ms": median_ms(total_ours(1)), "literal_ms": median_ms(total_literal(1))},
       "two_calls": {"ours_ms": median_ms(total_ours(2)), "literal_ms": median_ms(total_literal(2))},
       "per_call": {"conv_ms": median_ms(conv), "tail_ours_ms": median_ms(tail_ours),
                    "tail_literal_ms": median_ms(tail_literal), "ref_side_ours_ms": median_ms(ref_ours),
                    "ref_side_literal_ms": median_ms(ref_literal)}}
line = json.dumps(res)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
