"""Record tests/golden/loss_sums_parent.npz: what a given build of libacfm_hip.so answers to the one-launch forms of the
masked texture MSE and the silhouette losses (ops.tex_mse, ops.mask_losses: acfm_tex_mse, acfm_mask_losses given tickets,
whose sums are added in a fixed order) on seeded inputs -- the fixture tests/test_gpu_loss_bits_parent.py compares later
builds with, bit for bit.

    ACFM_LIB=PATH/libacfm_hip.so python tools/record_loss_parent.py [--out tests/golden/loss_sums_parent.npz]

Run it with the library of the commit BEFORE a change to k_tex_mse or k_mask_losses.  Only the outputs are stored; the
inputs are made again from the seeds below (numpy's default_rng: the same numbers on every machine).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (N, ref_batch, H, W, mask): 16-byte path, 80 px, per-pixel path, shared references, two workgroups of the narrow form,
# the wide form (8192 px per workgroup) with colours fetched in both rounds of four pieces
CASES = [(2, 2, 16, 16, "blob"), (3, 3, 8, 10, "one"), (2, 2, 7, 9, "checker"), (4, 2, 64, 64, "checker"),
         (1, 1, 96, 96, "blob"), (256, 256, 96, 96, "blob"), (256, 128, 96, 96, "sparse")]


def make_case(i, N, RB, H, W, kind):
    """-> tex [N,3,H,W], img [RB,3,H,W], mask [RB,H,W] (reference mask of the MSE), pred [N,H,W] (rendered mask of the
    silhouette losses: zero on most of the frame), gt [RB,H,W], edt [RB,1,H,W]; float32."""
    rng = np.random.default_rng(9000 + i)
    tex = rng.uniform(size=(N, 3, H, W)).astype(np.float32)
    img = rng.uniform(size=(RB, 3, H, W)).astype(np.float32)
    yy, xx = np.mgrid[:H, :W]
    if kind == "one":
        m = np.ones((RB, H, W), np.float32)
    elif kind == "checker":
        m = np.broadcast_to(((yy + xx) & 1).astype(np.float32), (RB, H, W)).copy()
    elif kind == "sparse":
        m = (rng.uniform(size=(RB, H, W)) > 0.98).astype(np.float32) * rng.uniform(0.1, 1.0, size=(RB, H, W)).astype(np.float32)
    else:
        cy, cx = rng.uniform(0.3, 0.7, size=(2, RB, 1, 1))
        r2 = ((yy[None] - cy * H) / (0.3 * H)) ** 2 + ((xx[None] - cx * W) / (0.25 * W)) ** 2
        m = np.clip(1.2 - r2, 0.0, 1.0).astype(np.float32)
    idx = np.arange(N) % RB
    pred = (m[idx] * rng.uniform(0.5, 1.0, size=(N, H, W))).astype(np.float32)
    gt = (rng.uniform(size=(RB, H, W)) > 0.5).astype(np.float32)
    edt = (rng.uniform(size=(RB, 1, H, W)) * 4).astype(np.float32)
    return tex, img, m, pred, gt, edt


def run_case(i, case):
    """-> (tex_mse [N], mask_losses [N,4]) of the loaded library, as numpy arrays."""
    import torch
    sys.path.insert(0, ROOT)
    from acfm_video_3d_reconstruction_amd import ops
    d = torch.device("cuda:0")
    tex, img, m, pred, gt, edt = (torch.tensor(x, device=d) for x in make_case(i, *case))
    return ops.tex_mse(tex, img, m).cpu().numpy(), ops.mask_losses(pred, gt, edt).cpu().numpy()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "loss_sums_parent.npz"))
    a = ap.parse_args()
    out = {}
    for i, case in enumerate(CASES):
        out["tex_%d" % i], out["ml_%d" % i] = run_case(i, case)
    np.savez(a.out, **out)
    print("wrote", a.out, {k: v.shape for k, v in out.items()})
