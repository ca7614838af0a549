#!/usr/bin/env python3
"""Host-only model of the atlas gradient's walk (k_tex_bwd_faces): how many serial load rounds a wave makes over the
pixel boxes of its faces, on the benchmark's cameras and the undeformed template.  Needs no GPU.

    python tools/texgrad_rounds.py [--mesh bird] [--frames 64] [--img 256] [--fpw 4] [--u 2]

The model takes front-facing faces as visible (no occlusion) and tight pixel boxes (the pixel centres inside the
face's bounding box), and deals the faces q, q + Q, .. of a mesh to wave q as the kernel does.  It prints the box sizes
and, per wave, the data rounds of
  * the walk before round 6: the first 64 pixels of each face side by side, then the rest face by face, 128 per round;
  * the walk since: the wave's boxes as one item list, 64 U items per round.
It is a model, not a measurement: profiles/r06_atlas_grad_ab.txt has the kernel's times.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from acfm_video_3d_reconstruction_amd.synthetic import batch_verts, make_cams  # noqa: E402


def rotate(q, x):
    """Rotate x [N,V,3] by the unit quaternions q [N,4] (w, x, y, z)."""
    w, u = q[:, None, :1], q[:, None, 1:]
    t = 2.0 * np.cross(u, x)
    return x + w * t + np.cross(u, t)


def box_pixels(verts, faces, cams, H):
    """-> cnt [N,F]: pixels in the tight box of every front-facing face, 0 for the others."""
    p = cams[:, None, :1] * rotate(cams[:, 3:7], verts)
    xy = -(p[..., :2] + cams[:, None, 1:3])                      # NDC of the texture branch: both axes flipped
    t = xy[:, faces]                                             # [N,F,3,2]
    e1, e2 = t[:, :, 1] - t[:, :, 0], t[:, :, 2] - t[:, :, 0]
    area = e1[..., 0] * e2[..., 1] - e1[..., 1] * e2[..., 0]
    front = area < 0          # the sign every face has that the CPU oracle's texture render shows
    lo, hi = t.min(2), t.max(2)
    a = np.ceil((lo + 1.0) * H / 2.0 - 0.5).astype(np.int64)     # first / last pixel centre inside the box
    b = np.floor((hi + 1.0) * H / 2.0 - 0.5).astype(np.int64)
    a, b = np.clip(a, 0, H), np.clip(b, -1, H - 1)
    wh = np.clip(b - a + 1, 0, None)
    return np.where(front, wh[..., 0] * wh[..., 1], 0)


def rounds(cnt, fpw, u):
    """cnt [N,F] -> (rounds of the old walk, rounds of the item list) per wave, [N,Q] each."""
    N, F = cnt.shape
    Q = (F + fpw - 1) // fpw
    c = np.zeros((N, fpw * Q), np.int64)
    c[:, :F] = cnt
    c = c.reshape(N, fpw, Q)                                     # wave q: faces q, q + Q, ..
    old = (c.max(1) > 0) + np.ceil(np.clip(c - 64, 0, None) / 128.0).sum(1)
    new = np.ceil(c.sum(1) / (64.0 * u))
    return old.astype(np.int64), new.astype(np.int64), c.sum(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", default="bird")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--img", type=int, default=256)
    ap.add_argument("--fpw", type=int, default=4)
    ap.add_argument("--u", type=int, default=2)
    a = ap.parse_args()
    m = np.load(os.path.join(ROOT, "tests", "golden", "meshes.npz"))
    v, f = m[a.mesh + "_v"], m[a.mesh + "_f"]
    rng = np.random.default_rng(1000)
    verts = batch_verts(v, a.frames, rng, 0.0)
    cams = make_cams(a.frames, rng, extent=float(np.abs(v).max()))
    cnt = box_pixels(verts.astype(np.float64), f, cams.astype(np.float64), a.img)
    vis = cnt[cnt > 0]
    print("%s, %d frames @%d: %d faces, %.0f %% front-facing with a pixel" % (a.mesh, a.frames, a.img, f.shape[0], 100.0 * vis.size / cnt.size))
    print("box pixels: median %d, mean %.0f, p90 %d, p99 %d, largest %d; more than 64: %.0f %% of the visible faces" % (
        np.median(vis), vis.mean(), np.percentile(vis, 90), np.percentile(vis, 99), vis.max(), 100.0 * (vis > 64).mean()))
    old, new, tot = rounds(cnt, a.fpw, a.u)
    print("box pixels per mesh %.1f k, per launch %.2f M" % (tot.sum(1).mean() / 1e3, tot.sum() / 1e6))
    for name, r in (("face by face (before round 6)", old), ("one list, %d items per round" % (64 * a.u), new)):
        print("data rounds per wave, %-32s mean %.2f, p99 %d, worst %d" % (name + ":", r.mean(), np.percentile(r, 99), r.max()))


if __name__ == "__main__":
    main()
