"""Record tests/golden/walk_parent.npz: what a given build of libacfm_hip.so renders on small scenes made to put a
known number of candidates into ONE 8x8 block -- the fixture tests/test_gpu_walk_fill.py compares later builds with,
bit for bit.

    python tools/record_walk_parent.py --lib PATH/libacfm_hip.so [--out tests/golden/walk_parent.npz]

Run it with the library of the commit BEFORE a change to bin_and_walk / walk_wave (csrc/acfm_raster.hip).  --lib is
put into ACFM_LIB before the package is imported, so the package's own operators run on that build.

The scenes (make_scene): `cand` small triangles with distinct depths inside a 6x6-pixel region of one block, and
decoy triangles in the other blocks of the same 16x16 coarse tile, mixed into the face order at random.  The decoys
are in the coarse tile's id list but fail the block's box, so the survivors of a binning round are spread over its 64
ids and a list that fills up does so in the middle of a round.  One face = three vertices of its own.  The camera is
the identity (scale 1, no shift, unit quaternion): a pixel centre c (in pixels) is world x = 2 c / H - 1.
candidates_in_block() counts, on the host and with k_setup's float32 arithmetic, the faces whose box (+ sqrt(blur))
meets the block: the number a scene is built for.

Recorded per scene: the inputs; of the K = 20 silhouette render the mask, the K-th keys (where the mask is not zero), all 20 id planes; of the
cover plane (the nearest covering face per pixel that the silhouette render leaves in its workspace) what a texture
render that takes that workspace over makes of it (image, silhouette, pix_to_face: it neither bins nor walks); of the
deterministic (fixed-point) backward grad_verts and grad_cams.  None of these depends on the order in which the
candidates are walked, so a build that chunks the candidate list differently must reproduce every bit.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLUR = float(np.log(1.0 / 1e-4 - 1.0) * 1e-4)
RBLK, CTILE = 8, 16

# name: (H, N, candidates, decoys, target block (by, bx), split mode or None)
#   24 | 25: the old walk threshold of the K = 20 list (88 - 64); 63..65: one round / the backward's 64 slots;
#   87..89: the K = 20 list; 128, 176, 177: two lists (2 x 64, 2 x 88 and one more); h20: image side no multiple of 8,
#   the block is cut by the image edge; n8: eight meshes (one per XCD group); direct: more than 512 ids in the coarse
#   tile (the id list is bypassed, the cursor is a face id); split: the block rendered by four workgroups.
CASES = {}
for _c in (24, 25, 63, 64, 65, 87, 88, 89):
    CASES["c%d" % _c] = (16, 1, _c, 3 * _c, (0, 0), None)
for _c in (128, 176, 177):
    CASES["c%d" % _c] = (16, 1, _c, _c, (0, 0), None)
CASES["h20_c89"] = (20, 1, 89, 180, (2, 1), None)
CASES["n8_c89"] = (16, 8, 89, 267, (1, 1), None)
CASES["direct_c201"] = (16, 1, 201, 399, (0, 1), None)
CASES["split_c177"] = (16, 1, 177, 177, (1, 0), 1)


def _region(b, H):
    """Pixel-centre range of the 6 inner pixels of block index b, cut at the image edge."""
    return RBLK * b + 1.5, min(RBLK * b + 6.5, H - 0.5)


def make_scene(name):
    """-> verts [N, 3F, 3] f32, faces [F, 3] i64, cams [N, 7] f32, is_target [F] bool."""
    H, N, cand, decoys, (by, bx), _ = CASES[name]
    rng = np.random.default_rng(sum(name.encode()) * 7919 + cand)
    F = cand + decoys
    is_target = np.zeros(F, bool)
    is_target[rng.permutation(F)[:cand]] = True
    cy, cx = by // 2, bx // 2
    others = [(y, x) for y in (2 * cy, 2 * cy + 1) for x in (2 * cx, 2 * cx + 1)
              if (y, x) != (by, bx) and RBLK * y < H and RBLK * x < H]
    verts = np.zeros((N, 3 * F, 3), np.float32)
    for n in range(N):
        z = rng.permutation(F).astype(np.float64) / F - 0.5          # distinct depths, unrelated to the face order
        for f in range(F):
            yb, xb = (by, bx) if is_target[f] else others[rng.integers(len(others))]
            (y0, y1), (x0, x1) = _region(yb, H), _region(xb, H)
            while True:
                c = np.array([rng.uniform(x0, x1), rng.uniform(y0, y1)])
                p = np.clip(c + rng.uniform(-2.5, 2.5, (3, 2)), [x0, y0], [x1, y1])
                area = (p[1, 0] - p[0, 0]) * (p[2, 1] - p[0, 1]) - (p[1, 1] - p[0, 1]) * (p[2, 0] - p[0, 0])
                if abs(area) > 0.05:                                    # pixels^2: far from degenerate
                    break
            verts[n, 3 * f:3 * f + 3, :2] = (2.0 * p / H - 1.0).astype(np.float32)
            verts[n, 3 * f:3 * f + 3, 2] = (z[f] + rng.uniform(-0.2, 0.2, 3) / F).astype(np.float32)
    faces = np.arange(3 * F, dtype=np.int64).reshape(F, 3)
    cams = np.tile(np.array([1, 0, 0, 1, 0, 0, 0], np.float32), (N, 1))
    return verts, faces, cams, is_target


def candidates_in_block(verts, faces, H, by, bx, blur=BLUR):
    """Per mesh: faces whose box, widened by sqrt(blur), meets the pixel centres of block (by, bx), and the ids of the
    block's coarse tile (faces meeting its 16x16 pixels) -- float32, the operations of k_setup and bin_and_walk."""
    f32 = np.float32
    ndc = -verts[..., :2].astype(f32)                                   # identity camera: NDC x, y = -world x, y
    tri = ndc[:, faces]                                                 # [N, F, 3, 2]
    m = f32(np.sqrt(f32(blur)))
    lo, hi = tri.min(2) - m, tri.max(2) + m

    def ndc_of(i):                                                      # pix_to_ndc(H - 1 - i, H)
        return f32(-1.0) + (f32(2.0) * f32(H - 1 - i) + f32(1.0)) / f32(H)

    def meets(p0, p1, q0, q1):                                          # pixel ranges [p0, p1] x [q0, q1] (y, x)
        xmax, xmin, ymax, ymin = ndc_of(q0), ndc_of(q1), ndc_of(p0), ndc_of(p1)
        return ~((xmin > hi[..., 0]) | (xmax < lo[..., 0]) | (ymin > hi[..., 1]) | (ymax < lo[..., 1]))

    blk = meets(RBLK * by, RBLK * by + 7, RBLK * bx, RBLK * bx + 7)
    cy, cx = by // 2, bx // 2
    # (the coarse mask is a superset: a face enters it by its box clamped to the image)
    coarse = meets(CTILE * cy, min(CTILE * cy + 15, H - 1), CTILE * cx, min(CTILE * cx + 15, H - 1))
    return blk.sum(1), coarse.sum(1)


def atlas_of(name, N, F):
    rng = np.random.default_rng(len(name) + 31 * F)
    return rng.uniform(0, 1, (N, F, 2, 2, 3)).astype(np.float32)


def grad_mask_of(name, N, H):
    rng = np.random.default_rng(len(name) + 17 * H)
    return (rng.standard_normal((N, H, H)) / (H * H)).astype(np.float32)


def run_case(name, verts, faces, cams):
    """The loaded library's answers for one scene -> dict of numpy arrays (the recorded outputs)."""
    import torch
    from acfm_video_3d_reconstruction_amd import _lib, ops
    H, N, _, _, _, split = CASES[name]
    d = torch.device("cuda:0")
    kw = {} if split is None else {"split": split}
    tf = torch.from_numpy(faces).to(d)
    g = torch.from_numpy(grad_mask_of(name, N, H)).to(d)
    atlas = torch.from_numpy(atlas_of(name, N, faces.shape[0])).to(d)
    with _lib.raster_tuning(deterministic=True, record_cover=True, **kw):
        tv = torch.tensor(verts, device=d, requires_grad=True)
        tc = torch.tensor(cams, device=d, requires_grad=True)
        mask, p2f = ops.sil_render(tv, tf, tc, H)
        kth = mask.grad_fn.saved_tensors[4]                             # the K-th keys (u64 bits in an int64 tensor)
        assert kth.dtype == torch.int64 and tuple(kth.shape) == (N, H, H)
        # (defined where the mask is not zero: the backward reads it nowhere else, and a block flagged empty stores none)
        kth = torch.where(mask.detach() != 0, kth, torch.zeros_like(kth))
        # the same tensors: the texture render takes the silhouette render's workspace over and shades from its cover plane
        imgs, sil, tp2f = ops.tex_render(tv, tf, tc, atlas, H)
        (mask * g).sum().backward()
        torch.cuda.synchronize()
    out = {"mask": mask.detach(), "kth": kth, "p2f": p2f, "cover_img": imgs.detach(), "cover_sil": sil.detach(),
           "cover_p2f": tp2f, "grad_verts": tv.grad, "grad_cams": tc.grad}
    out = {k: v.cpu().numpy() for k, v in out.items()}
    out["p2f"] = out["p2f"].astype(np.int32)                            # ids < 2^31: half the file
    out["cover_p2f"] = out["cover_p2f"].astype(np.int32)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "walk_parent.npz"))
    a = ap.parse_args()
    os.environ["ACFM_LIB"] = os.path.abspath(a.lib)
    sys.path.insert(0, ROOT)
    out = {}
    for name, (H, N, cand, decoys, (by, bx), _) in CASES.items():
        verts, faces, cams, _ = make_scene(name)
        nb, nc = candidates_in_block(verts, faces, H, by, bx)
        assert (nb == cand).all(), (name, nb)
        res = run_case(name, verts, faces, cams)
        assert (res["p2f"][..., 0] >= 0).any() and np.abs(res["grad_verts"]).max() > 0
        out[name + "/verts"], out[name + "/faces"], out[name + "/cams"] = verts, faces.astype(np.int32), cams
        for k, x in res.items():
            out[name + "/" + k] = x
        print("%-12s H=%d N=%d F=%d candidates=%d coarse ids=%d covered=%d kept=%d" % (
            name, H, N, faces.shape[0], cand, nc[0], (res["p2f"][..., 0] >= 0).sum(), (res["p2f"] >= 0).sum()))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **out)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
