#!/usr/bin/env python3
"""Host model of how bin_and_walk (csrc/acfm_raster.hip) cuts a block's candidates into walks, on the headline batch
of tools/count_events.py (bird, 64 frames @256^2, seed 1000, batch_verts(.., 0.005), blur ln(9999) 1e-4): numpy only.

    python tools/walk_chunk_model.py [--fwd-cap 88] [--bwd-cap 64] [--frames 64] [--img 256] [--no-edge-cull]

Per mesh: face boxes widened by sqrt(blur); per 16x16 coarse tile the ids of the faces meeting it, ascending; per 8x8
block rounds of 64 ids (more than 512 ids: all faces, the `direct` path), the survivors of the block's box appended
to a list of CAP slots and walked
  today  : when the list holds more than CAP - 64 (the next round could overflow it), or at the end;
  filled : when it holds CAP -- a round appends what fits and the next round starts at the first survivor left over.
A walk costs max over the four 4x4 groups of their sub-list lengths (forward: by box and, unless --no-edge-cull, the
edge-line test of edge_cull4), or for the backward max over the two pairs (longest with shortest, the middle two) of
ceil((n_a + n_b) / 2) (walk_wave<.., SHARE>; sub-lists by box only).  Printed: walk calls, candidates and walk
iterations of both rules, for the backward (it walks only blocks with a non-zero gradient: modelled as every block
with candidates, as the counting build's 374 k against this model's 375.6 k justify) and the K = 20 forward, and the
forward's blocks with at least 160 candidates -- the launch's critical path -- alone.  tools/count_events.py prints
the same quantities counted on the GPU by the ACFM_DIAG_COUNT build.
"""
import argparse
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RBLK, CTILE, FLCAP, RT = 8, 16, 512, 64


def _synthetic():
    # by path: the package's __init__ imports torch, this tool needs numpy only
    spec = importlib.util.spec_from_file_location(
        "synthetic", os.path.join(ROOT, "acfm_video_3d_reconstruction_amd", "synthetic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def project_ndc(verts, cams):
    """orthographic_proj_withz + the renderer's view: NDC x, y = -(s R(q) X + t)."""
    q = cams[:, None, 3:7].astype(np.float64)
    X = verts.astype(np.float64)
    w, u = q[..., :1], q[..., 1:]
    t = 2.0 * np.cross(u, X)
    r = X + w * t + np.cross(u, t)                                   # unit quaternion rotation
    xy = cams[:, None, :1] * r[..., :2] + cams[:, None, 1:3]
    return -xy


def chunks(passing, cap, filled):
    """passing: bool over the id list.  -> list of index arrays (positions in the id list), one per walk."""
    out, lst, i, n = [], [], 0, len(passing)
    while i < n:
        r = i + np.flatnonzero(passing[i:i + RT])
        if filled:
            room = cap - len(lst)
            if len(r) > room:
                lst.extend(r[:room]); i = int(r[room])
            else:
                lst.extend(r); i += RT
            if len(lst) == cap:
                out.append(np.asarray(lst)); lst = []
        else:
            lst.extend(r); i += RT
            if len(lst) > cap - RT:
                out.append(np.asarray(lst)); lst = []
    if lst:
        out.append(np.asarray(lst))
    return out


def edge_far(tri, cx, cy, hx, hy, r):
    """edge_cull4: tri [n, 3, 2]; -> bool [n]: the block (centre cx, cy, half extents hx, hy) lies farther than r outside
    one edge line."""
    far = np.zeros(len(tri), bool)
    for e in range(3):
        q, o = (e + 1) % 3, (e + 2) % 3
        nx, ny = tri[:, q, 1] - tri[:, e, 1], tri[:, e, 0] - tri[:, q, 0]
        side = nx * (tri[:, o, 0] - tri[:, e, 0]) + ny * (tri[:, o, 1] - tri[:, e, 1])
        nx, ny = np.where(side > 0, -nx, nx), np.where(side > 0, -ny, ny)
        thr2 = r * r * (nx * nx + ny * ny)
        m = nx * (cx - tri[:, e, 0]) + ny * (cy - tri[:, e, 1]) - (np.abs(nx) * hx + np.abs(ny) * hy)
        far |= (m > 0) & (m * m > thr2)
    return far


def fwd_cost(n):
    return int(max(n))


def bwd_cost(n):
    s = sorted(n)
    return max((s[3] + s[0] + 1) // 2, (s[2] + s[1] + 1) // 2)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--fwd-cap", type=int, default=88)
    ap.add_argument("--bwd-cap", type=int, default=64)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--img", type=int, default=256)
    ap.add_argument("--no-edge-cull", action="store_true")
    ap.add_argument("--heavy", type=int, default=160, help="candidates from which a forward block counts as heavy")
    a = ap.parse_args()
    syn = _synthetic()
    m = np.load(os.path.join(ROOT, "tests", "golden", "meshes.npz"))
    v, f = m["bird_v"], m["bird_f"]
    rng = np.random.default_rng(1000)
    N, H = a.frames, a.img
    verts = syn.batch_verts(v, N, rng, 0.005)
    cams = syn.make_cams(N, rng, extent=float(np.abs(v).max()))
    blur = float(np.log(1.0 / 1e-4 - 1.0) * 1e-4)
    margin = np.sqrt(blur)
    r_cull = margin * 1.001
    ndc = project_ndc(verts, cams)
    F = f.shape[0]
    nb, nc = (H + RBLK - 1) // RBLK, (H + CTILE - 1) // CTILE

    def centre(i):                                                   # pix_to_ndc(H - 1 - i, H)
        return 1.0 - (2.0 * np.asarray(i, np.float64) + 1.0) / H

    def meets(lo, hi, first, last):                                  # [F] boxes against pixel ranges [first, last] -> [len, F]
        cmax, cmin = centre(first)[:, None], centre(last)[:, None]
        return ~((cmin > hi[None]) | (cmax < lo[None]))

    b0, c0, g0 = np.arange(nb) * RBLK, np.arange(nc) * CTILE, np.arange(2 * nb) * 4
    keys = ("calls", "cand", "iters")
    tot = {(k, w, r): 0 for k in ("bwd", "fwd", "fwd_heavy") for w in keys for r in (0, 1)}
    heavy_blocks = 0
    for n in range(N):
        tri = ndc[n][f]                                              # [F, 3, 2]
        lo, hi = tri.min(1) - margin, tri.max(1) + margin
        area = (tri[:, 1, 0] - tri[:, 0, 0]) * (tri[:, 2, 1] - tri[:, 0, 1]) - (tri[:, 1, 1] - tri[:, 0, 1]) * (tri[:, 2, 0] - tri[:, 0, 0])
        live = np.abs(area) > 1e-8                                   # a degenerate face's box meets nothing
        bx, by = meets(lo[:, 0], hi[:, 0], b0, b0 + 7) & live, meets(lo[:, 1], hi[:, 1], b0, b0 + 7) & live
        cx = meets(lo[:, 0], hi[:, 0], c0, np.minimum(c0 + 15, H - 1)) & live
        cy = meets(lo[:, 1], hi[:, 1], c0, np.minimum(c0 + 15, H - 1)) & live
        gx, gy = meets(lo[:, 0], hi[:, 0], g0, g0 + 3), meets(lo[:, 1], hi[:, 1], g0, g0 + 3)
        for ty in range(nb):
            for tx in range(nb):
                hit = by[ty] & bx[tx]
                if not hit.any():
                    continue
                ids = np.flatnonzero(cy[ty // 2] & cx[tx // 2])
                if len(ids) > FLCAP:
                    ids = np.arange(F)                               # `direct`: the faces themselves, 64 at a time
                passing = hit[ids]
                ncand = int(passing.sum())
                gbox = [gy[2 * ty + (g >> 1)] & gx[2 * tx + (g & 1)] for g in range(4)]
                gc = [(centre(RBLK * tx + 4 * (g & 1)) + centre(RBLK * tx + 4 * (g & 1) + 3)) / 2 for g in range(4)]
                gr = [(centre(RBLK * ty + 4 * (g >> 1)) + centre(RBLK * ty + 4 * (g >> 1) + 3)) / 2 for g in range(4)]
                for filled in (0, 1):
                    for kind, cap in (("bwd", a.bwd_cap), ("fwd", a.fwd_cap)):
                        for ch in chunks(passing, cap, filled):
                            fc = ids[ch]
                            if kind == "fwd" and not a.no_edge_cull:
                                cnt = [int((gbox[g][fc] & ~edge_far(tri[fc], gc[g], gr[g], 3.0 / H, 3.0 / H, r_cull)).sum())
                                       for g in range(4)]
                            else:
                                cnt = [int(gbox[g][fc].sum()) for g in range(4)]
                            it = bwd_cost(cnt) if kind == "bwd" else fwd_cost(cnt)
                            for k in ((kind,) if kind == "bwd" or ncand < a.heavy else (kind, "fwd_heavy")):
                                tot[(k, "calls", filled)] += 1
                                tot[(k, "cand", filled)] += len(fc)
                                tot[(k, "iters", filled)] += it
                heavy_blocks += ncand >= a.heavy
    print("bird, %d frames @%d^2, seed 1000; list capacities: backward %d, K = 20 forward %d%s" % (
        N, H, a.bwd_cap, a.fwd_cap, "; forward sub-lists by box only" if a.no_edge_cull else "; forward sub-lists by box + edge lines"))
    print("%-44s %10s %10s %8s   %12s %12s %8s" % ("", "calls", "filled", "", "iterations", "filled", ""))
    for k, label in (("bwd", "backward"), ("fwd", "K = 20 forward"),
                     ("fwd_heavy", "forward, the %d blocks with >= %d candidates" % (heavy_blocks, a.heavy))):
        c0_, c1_, i0_, i1_ = tot[(k, "calls", 0)], tot[(k, "calls", 1)], tot[(k, "iters", 0)], tot[(k, "iters", 1)]
        print("%-44s %10d %10d %+7.1f%%   %12d %12d %+7.1f%%   (candidates %d)" % (
            label, c0_, c1_, 100.0 * (c1_ - c0_) / max(c0_, 1), i0_, i1_, 100.0 * (i1_ - i0_) / max(i0_, 1), tot[(k, "cand", 0)]))
        assert tot[(k, "cand", 0)] == tot[(k, "cand", 1)]


if __name__ == "__main__":
    main()
