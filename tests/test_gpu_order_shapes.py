"""GPU: the heavy-first order (k_order) with one workgroup per (XCD group, mesh).  Silhouette render + backward and the
texture render against the oracle -- face ids bit for bit, masks 1e-6, gradients at the bars of
tests/test_gpu_edge_cases.py -- over batches of eight groups (N % 8 == 0) and of one group, block counts per mesh that
are no multiple of the workgroup (tt = 25, 64, 289), more blocks than threads (tt = 1089: the loop), counters left in
global memory by the face setup (tt = 4225), 4, 8 and 16 face slices per mesh, the heaviest blocks split and not.
Every case runs twice: the order inside a cost class is free, the forward outputs are not."""
import numpy as np
import pytest
import torch

from acfm_video_3d_reconstruction_amd.synthetic import batch_verts, make_cams
from oracle import oracle as O

pytestmark = pytest.mark.gpu

# (mesh, N, H, split mode or None = automatic, backward checked)
#   face slices per mesh (RasterWs.slices): N >= 64 four, N >= 32 eight, fewer sixteen (k_order<true> joins the boxes)
CASES = [("bird", 8, 40, None, True), ("bird", 16, 64, None, True), ("bird", 24, 40, None, True),
         ("bird", 3, 64, None, True), ("bird", 5, 136, None, True), ("bird", 8, 136, None, True),
         ("bird", 3, 264, None, True), ("bird", 2, 520, None, False),
         ("horse", 32, 40, None, True), ("horse", 4, 64, None, True), ("bird", 64, 40, None, True),
         ("bird", 8, 64, 1, True), ("bird", 8, 64, 0, True), ("bird", 5, 40, 1, True),
         # more meshes than workgroups of the launch (128): two meshes per workgroup, the last one of a group with one
         ("bird", 136, 16, None, False), ("bird", 131, 16, None, False), ("bird", 272, 24, 1, False)]

ENTRY_EMPTY, ENTRY_SPLIT = 1 << 30, 1 << 29


def _order_of(ws, N, V, F, H, split):
    """The schedule k_order left in the raster workspace `ws` (uint8 tensor; layout: carve_ws of csrc/acfm_common.h):
    -> (tile_cnt [N,tt], order [N*tt], n_work [8], split_slots)."""
    a256 = lambda x: (x + 255) & ~255
    slices = 4 if N >= 64 else 8 if N >= 32 else 16
    while slices > 4 and (F + slices - 1) // slices < 64:
        slices >>= 1
    tt = ((H + 7) // 8) ** 2
    o = a256(12 * N * V) + a256(128 * N * F) + a256(16 * N * F) + a256(16 * slices * N) + a256(8 * N * V) + a256(16 * N * V)
    words = lambda off, n: ws[off:off + 4 * n].cpu().numpy().view(np.int32)
    cnt = words(o, N * tt).reshape(N, tt)
    o += a256(4 * N * tt) + a256(4 * slices * N * tt)
    order = words(o, N * tt)
    o += a256(4 * N * tt)
    n_work = words(o, 8)
    per_group = N // 8 if N % 8 == 0 else N
    mode = -5 if split is None else split
    if mode == 0:
        slots = 0
    elif mode > 0 or N * tt <= 40960:
        slots = min(per_group * 32, 1024)
    else:
        slots = min(per_group * 4, 256)
    return cnt, order, n_work, slots


def _cost_class(c):
    for k, lim in enumerate((240, 200, 160, 112, 80, 56, 36, 20, 1)):
        if c >= lim:
            return k
    return 9


def _check_order(ws, N, V, F, H, split):
    """Every group's order is a permutation of its entries in ascending cost class, the flagged-empty entries are exactly
    the blocks no face box comes near and end the order, n_work counts the others, and the split flag sits on the first
    entries of the order only, on classes that may split."""
    cnt, order, n_work, slots = _order_of(ws, N, V, F, H, split)
    G = 8 if N % 8 == 0 else 1
    tt = cnt.shape[1]
    per = (N // G) * tt
    flagged = 0
    for g in range(G):
        o = order[g * per:(g + 1) * per]
        e = o & ~(ENTRY_EMPTY | ENTRY_SPLIT)
        assert np.array_equal(np.sort(e), np.arange(per)), "not a permutation"
        cost = cnt[(e // tt) * G + g, e % tt]
        cls = np.array([_cost_class(int(c)) for c in cost])
        assert (np.diff(cls) >= 0).all(), "classes not ascending"
        assert np.array_equal((o & ENTRY_EMPTY) != 0, cost == 0)
        assert int(n_work[g]) == int((cost > 0).sum())
        sp = (o & ENTRY_SPLIT) != 0
        assert not sp[slots:].any() and (cls[sp] <= 4).all()
        if sp.any():
            assert sp[:int(sp.sum())].all()          # the first entries of the order, without a gap
        flagged += int(sp.sum())
    return flagged


@pytest.mark.parametrize("name,n,H,split,bwd", CASES)
def test_order_per_mesh_workgroups(meshes, name, n, H, split, bwd):
    from acfm_video_3d_reconstruction_amd import _lib, ops
    d = torch.device("cuda:0")
    rng = np.random.default_rng(500 + 7 * n + H)
    v, f = meshes[name + "_v"], meshes[name + "_f"]
    verts = batch_verts(v, n, rng, 0.01)
    cams = make_cams(n, rng, extent=float(np.abs(v).max()))
    cams[::3, 1:3] += 0.35                     # some meshes partly outside: the meshes of a group differ in their classes
    if split is not None:
        cams[:, 0] *= 0.35                     # small meshes: > 80 face boxes on their blocks (the classes that split)
    atlas = rng.uniform(0, 1, (n, f.shape[0], 2, 2, 3)).astype(np.float32)
    g = (rng.standard_normal((n, H, H)) / (H * H)).astype(np.float32)
    ref_mask, ref_p2f = O.sil_render(verts, f, cams, H)
    ref_img, ref_sil, ref_p2, _ = O.tex_render(verts, f, cams, atlas, H)
    if bwd:
        gv, gc, _, _ = O.sil_render_backward(verts, f, cams, H, g)
    assert (ref_p2f[..., 0] >= 0).mean() > 0.005
    tf, ta = torch.from_numpy(f).to(d), torch.tensor(atlas, device=d)
    runs = []
    for rep in range(2):
        ops._SETUP.clear()
        tv = torch.tensor(verts, device=d, requires_grad=True)
        tc = torch.tensor(cams, device=d, requires_grad=True)
        with _lib.raster_tuning(**({} if split is None else {"split": split})):
            mask, p2f = ops.sil_render(tv, tf, tc, H)
            if rep == 0:
                ent = ops._shared_setup(tv.detach(), tc.detach(), ops.expand_faces(tf, n), H, 0.0)
                assert ent is not None
                flagged = _check_order(ent[0], n, verts.shape[1], f.shape[0], H, split)
                assert (flagged > 0) if split == 1 else (flagged == 0 if split == 0 else True)
            if bwd:
                (mask * torch.tensor(g, device=d)).sum().backward()
            imgs, sil, p2 = ops.tex_render(tv.detach(), tf, tc.detach(), ta, H)
        runs.append((mask.detach(), p2f, imgs, sil, p2))
        if rep:
            continue
        np.testing.assert_array_equal(p2f.cpu().numpy(), ref_p2f)
        np.testing.assert_allclose(mask.detach().cpu().numpy(), ref_mask, rtol=0, atol=1e-6)
        np.testing.assert_array_equal(p2.cpu().numpy(), ref_p2)
        np.testing.assert_allclose(imgs.cpu().numpy(), ref_img, rtol=0, atol=1e-6)
        np.testing.assert_allclose(sil.cpu().numpy(), ref_sil, rtol=0, atol=1e-6)
        if bwd:
            sv, sc = max(np.abs(gv).max(), 1e-20), max(np.abs(gc).max(), 1e-20)
            np.testing.assert_allclose(tv.grad.cpu().numpy(), gv, rtol=1e-4, atol=1e-4 * sv)
            np.testing.assert_allclose(tc.grad.cpu().numpy(), gc, rtol=1e-4, atol=1e-4 * sc)
            for got, want in ((tv.grad.cpu().numpy(), gv), (tc.grad.cpu().numpy(), gc)):
                rel = np.linalg.norm(got.astype(np.float64) - want) / max(np.linalg.norm(want.astype(np.float64)), 1e-30)
                assert rel < 1e-5, rel
    for a, b in zip(*runs):
        assert torch.equal(a, b)
