"""Record tests/golden/atlas_grad_parent.npz: the atlas gradient that a given build of libacfm_hip.so returns for the
hand-built scenes below, on both entry paths of the gather kernel k_tex_bwd_faces (an explicit image gradient:
acfm_tex_backward_faces; masked_texture_mse on the rendered image: acfm_tex_mse_backward_faces) -- the fixture
tests/test_gpu_atlas_grad_shapes.py compares later builds with, bit for bit.

    ACFM_LIB=PATH/libacfm_hip.so python tools/record_atlas_grad_parent.py [--out tests/golden/atlas_grad_parent.npz]

Run it with the library of the commit BEFORE a change to k_tex_bwd_faces.  Only the gradients are stored; scenes and
inputs are made again from the code and seeds below (numpy's default_rng: the same numbers on every machine).

The scenes are triangles in the image plane under the identity camera (vertex (x, y) = minus the NDC position, larger
z = farther), every face with vertices of its own.  A wave of the kernel takes the faces f0, f0 + Q, f0 + 2Q, f0 + 3Q
(Q = ceil(F / 4)), so face numbers below are chosen by wave.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENTITY_CAM = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)

# (scene, N, NA, H, R, shared): shared = the texture render takes over the workspace of a silhouette render with
# blur > 0 (the box_shrink path).  NA = 8 takes the per-XCD placement, NA = 3 does not; N = 2 NA: two hypotheses
# of a frame share its atlas.
CASES = [("mixed", 8, 8, 40, 6, False),
         ("mixed", 6, 3, 37, 8, False),
         ("mixed", 16, 8, 37, 1, True),
         ("few", 3, 3, 40, 6, False),
         ("mixed", 3, 3, 40, 6, True)]


def _tri(cx, cy, r, z, rot=0.0):
    a = rot + np.array([np.pi / 2, np.pi / 2 + 2 * np.pi / 3, np.pi / 2 + 4 * np.pi / 3])
    return np.stack([cx + r * np.cos(a), cy + r * np.sin(a), np.full(3, z)], 1)


def make_scene(kind, N, seed):
    """-> verts [N, 3F, 3] float32, faces [F, 3] int64.  Every mesh is the same layout, jittered a little."""
    rng = np.random.default_rng(seed)
    if kind == "few":                 # F = 3 < faces per wave: a big, a small and a medium face
        tris = [_tri(0.0, 0.0, 0.9, 1.0), _tri(0.5, 0.5, 0.12, 0.5), _tri(-0.4, -0.3, 0.35, 0.6, 0.4)]
    else:
        F = 26                        # not a multiple of 4; Q = 7
        tris = [None] * F
        # wave 0 (faces 0, 7, 14, 21): all big.  Face 0 covers the whole image from the back (its box reaches far
        # outside the image and is clipped to H^2 pixels: more than three rounds of the walk).
        tris[0] = np.array([[-4.0, -3.0, 2.0], [4.0, -3.0, 2.0], [0.0, 6.0, 2.0]])
        tris[7] = _tri(-0.35, 0.3, 0.6, 1.0)
        tris[14] = _tri(0.4, -0.35, 0.55, 0.9, 0.5)
        tris[21] = _tri(0.3, 0.45, 0.45, 0.8, 1.0)
        # wave 1 (faces 1, 8, 15, 22): big, small, invisible (behind face 0), small
        tris[1] = _tri(-0.45, -0.45, 0.5, 0.7, 0.2)
        tris[8] = _tri(0.8, 0.8, 0.08, 0.3)
        tris[15] = _tri(0.1, 0.1, 0.5, 3.0)
        tris[22] = _tri(-0.8, 0.75, 0.1, 0.3, 0.7)
        # wave 2 (faces 2, 9, 16, 23): degenerate (a point: empty / infinite box), wholly outside, partly outside, medium
        tris[2] = np.tile(np.array([[0.2, -0.1, 0.5]]), (3, 1))
        tris[9] = _tri(1.9, 0.2, 0.3, 0.5)
        tris[16] = _tri(0.95, -0.6, 0.3, 0.4, 0.3)
        tris[23] = _tri(-0.1, -0.75, 0.22, 0.4)
        # wave 3 (faces 3, 10, 17, 24): a thin sliver (a wide box, 72 pixels at H = 40: between 64 pixels and one round of
        # the walk, with few pixels of its own), a face hidden completely by face 24 in front of it, and a small one
        tris[3] = np.array([[-0.9, 0.05, 0.35], [0.9, 0.12, 0.35], [0.9, 0.16, 0.35]])
        tris[10] = _tri(-0.75, -0.8, 0.06, 0.6)
        tris[24] = _tri(-0.75, -0.8, 0.12, 0.2)               # hides face 10 completely
        tris[17] = _tri(0.65, 0.1, 0.09, 0.25, 0.9)
        k = 0
        for f in range(F):            # the rest: small faces on a grid, in front
            if tris[f] is None:
                tris[f] = _tri(-0.8 + 0.2 * (k % 9), -0.15 + 0.3 * (k // 9), 0.05 + 0.01 * (k % 4), 0.1 + 0.01 * k, 0.3 * k)
                k += 1
    v = np.concatenate(tris, 0)
    verts = np.tile(v[None], (N, 1, 1))
    verts[..., :2] += rng.uniform(-0.02, 0.02, size=(N, 1, 2)) + rng.uniform(-0.004, 0.004, size=(N, v.shape[0], 2))
    faces = np.arange(v.shape[0], dtype=np.int64).reshape(-1, 3)
    return verts.astype(np.float32), faces


def tight_boxes(verts, faces, H):
    """-> [N,F]: the pixels whose centre lies in the bounding box of each face (what the kernel walks, blur margin aside)."""
    t = -verts[:, faces][..., :2].astype(np.float64)
    lo, hi = t.min(2), t.max(2)
    a = np.clip(np.ceil((lo + 1.0) * H / 2.0 - 0.5), 0, H)
    b = np.clip(np.floor((hi + 1.0) * H / 2.0 - 0.5), -1, H - 1)
    wh = np.clip(b - a + 1, 0, None)
    return (wh[..., 0] * wh[..., 1]).astype(np.int64)


def make_inputs(i, case):
    """-> dict of float32 arrays: verts, faces, cams, atlas [NA,F,R,R,3], g [N,3,H,H] (explicit gradient), ref [NA,3,H,H],
    mask [NA,H,H] (soft, with a zero band and a zero half in every second frame), wts [N] (weights of the MSE terms)."""
    kind, N, NA, H, R, _ = case
    verts, faces = make_scene(kind, N, 7100 + i)
    rng = np.random.default_rng(7200 + i)
    F = faces.shape[0]
    mask = rng.uniform(0.2, 1.0, size=(NA, H, H)).astype(np.float32)
    mask[:, H // 3:H // 3 + 3] = 0.0
    mask[1::2, :, :H // 2] = 0.0
    return dict(verts=verts, faces=faces, cams=np.tile(np.array(IDENTITY_CAM, np.float32), (N, 1)),
                atlas=rng.uniform(0, 1, size=(NA, F, R, R, 3)).astype(np.float32),
                g=rng.standard_normal((N, 3, H, H)).astype(np.float32),
                ref=rng.uniform(0, 1, size=(NA, 3, H, H)).astype(np.float32), mask=mask,
                wts=rng.uniform(0.5, 2.0, size=N).astype(np.float32))


def run_case(i, case, calls=None):
    """Both paths on the loaded library -> dict: ga_given, ga_mse [NA,F,R,R,3], tidx [N,H,H] (the render's own texel
    indices), imgs [N,3,H,H] (the rendered image), as numpy arrays.  calls: a list that receives the names of the
    C entry points called."""
    import torch
    sys.path.insert(0, ROOT)
    from acfm_video_3d_reconstruction_amd import _lib, ops
    from acfm_video_3d_reconstruction_amd.nnutils import loss_utils as L
    kind, N, NA, H, R, shared = case
    x = make_inputs(i, case)
    d = torch.device("cuda:0")
    verts, cams = torch.tensor(x["verts"], device=d), torch.tensor(x["cams"], device=d)
    faces = torch.tensor(x["faces"], device=d)[None].repeat(N, 1, 1).contiguous()
    out = {}
    real_call = _lib.call

    def spy(name, *a, **k):
        if calls is not None:
            calls.append(name)
        return real_call(name, *a, **k)
    _lib.call = spy
    try:
        for path in ("given", "mse"):
            atlas = torch.tensor(x["atlas"], device=d, requires_grad=True)
            ops._SETUP.clear()
            if shared:
                ops.sil_render(verts, faces, cams, H)
                hit = ops._shared_setup(verts, cams, ops.expand_faces(faces, N), H, 0.0)
                assert hit is not None and hit[2] > 0           # the workspace is taken over, and its boxes carry a blur margin
            imgs, _, _ = ops.tex_render(verts, faces, cams, atlas, H)
            tidx = imgs.grad_fn.saved_tensors[0]
            if path == "given":
                (imgs * torch.tensor(x["g"], device=d)).sum().backward()
            else:
                mse = L.masked_texture_mse(imgs, torch.tensor(x["ref"], device=d), torch.tensor(x["mask"], device=d))
                (mse * torch.tensor(x["wts"], device=d)).sum().backward()
            out["ga_" + path] = atlas.grad.cpu().numpy()
            out["tidx"], out["imgs"] = tidx.cpu().numpy(), imgs.detach().cpu().numpy()
    finally:
        _lib.call = real_call
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "atlas_grad_parent.npz"))
    a = ap.parse_args()
    res = {}
    for i, case in enumerate(CASES):
        r = run_case(i, case)
        res["given_%d" % i], res["mse_%d" % i] = r["ga_given"], r["ga_mse"]
        cov = r["tidx"] >= 0
        print("case %d %s: covered %.2f, texels with gradient %d of %d" % (
            i, case, cov.mean(), (np.abs(r["ga_given"]).sum(-1) > 0).sum(), r["ga_given"][..., 0].size))
    np.savez_compressed(a.out, **res)
    print("wrote", a.out, {k: v.shape for k, v in res.items()})
