"""CPU: the model of half storage (tests/half_storage.py) pinned on the host -- its rounding against torch's, the
zero-mask agreement its backward rule rests on, its loss expressions against the oracle's and against autograd, and
the condition on the INPUTS of tests/test_gpu_half_storage.py that makes its backward comparison bite: on the scenes
used there the half mask changes 1 - m by more than a percent at soft pixels and wipes it out at others, and the
oracle's own gradient moves by a hundred times the bar between the two readings."""
import numpy as np
import pytest
import torch

import half_storage as M
import raster_scenes as S
from oracle import oracle as O
from test_gpu_half_storage import BWD_KS, TEETH, backward_scenes, upstream

f32 = np.float32


# ------------------------------------------------------------------------------------------------ rounding
def _grid():
    rng = np.random.default_rng(0)
    known = [0.0, 2.0 ** -24, 2.0 ** -25, 1 - 2.0 ** -12, 1 - 2.0 ** -11, 65504.0, 1.0, 0.5, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -25,
             3 * 2.0 ** -25, 5 * 2.0 ** -25, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 65519.0]
    x = np.concatenate([np.array(known, f32), np.nextafter(np.array(known, f32), f32(np.inf)),
                        np.nextafter(np.array(known, f32), f32(-np.inf)), rng.uniform(0, 1, 4096).astype(f32),
                        (2.0 ** rng.uniform(-30, 15.9, 4096)).astype(f32), np.linspace(0, 2.0 ** -13, 2049, dtype=f32)])
    return np.concatenate([x, -x])


def test_h_is_torchs_rounding():
    x = _grid()
    want = torch.from_numpy(x).half().float().numpy()
    got = M.h(x)
    assert got.dtype == f32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(M.stored(x).view(np.uint16), torch.from_numpy(x).half().numpy().view(np.uint16))
    # round to nearest EVEN, subnormals kept
    for v, r in ((2.0 ** -24, 2.0 ** -24), (2.0 ** -25, 0.0), (3 * 2.0 ** -25, 2.0 ** -23), (5 * 2.0 ** -25, 2.0 ** -23),
                 (1 - 2.0 ** -12, 1.0), (1 - 2.0 ** -11, 1 - 2.0 ** -11), (1 + 2.0 ** -11, 1.0), (1 + 3 * 2.0 ** -11, 1 + 2.0 ** -9),
                 (65504.0, 65504.0), (65519.0, 65504.0)):
        assert M.h(f32(v)) == f32(r), (v, r)
    assert M.h(np.nextafter(f32(2.0 ** -25), f32(1))) == f32(2.0 ** -24)
    assert M.stored(f32(0.0)).view(np.uint16) == 0 and M.stored(f32(-0.0)).view(np.uint16) == 0x8000


def test_stored_ids():
    p = np.array([[[[5, 7], [-1, -1]]]], np.int64)
    got = M.stored_ids(p)
    assert got.dtype == np.int32 and got.shape == (1, 1, 2, 1) and got.ravel().tolist() == [5, -1]


def test_zero_mask_agreement():
    """mask = 1 - alpha with alpha a float32 in [0, 1]: 0, or at least 2^-24, which half keeps."""
    rng = np.random.default_rng(1)
    one = f32(1.0)
    a = np.concatenate([np.array([0.0, 1.0, np.nextafter(one, f32(0)), np.nextafter(np.nextafter(one, f32(0)), f32(0)),
                                  0.5, np.nextafter(f32(0.5), one), 2.0 ** -24, 2.0 ** -30, 1e-38], f32),
                        rng.uniform(0, 1, 100000).astype(f32), one - (2.0 ** rng.uniform(-24, 0, 100000)).astype(f32),
                        (2.0 ** rng.uniform(-60, 0, 10000)).astype(f32)])
    assert ((a >= 0) & (a <= 1)).all()
    m = one - a
    assert m.dtype == f32 and ((m == 0) | (m >= f32(2.0 ** -24))).all()
    assert (one - np.nextafter(one, f32(0))) == f32(2.0 ** -24)
    assert M.h(f32(2.0 ** -24)) != 0
    assert M.zero_mask_agrees(m)
    assert not M.zero_mask_agrees(np.array([2.0 ** -25], f32))          # (what the helper would catch)
    r = M.ratio(m, M.h(m))
    assert r.dtype == f32 and np.isfinite(r).all() and (r >= 0).all() and (r <= 2).all()
    assert (r[m == 1] == 0).all() and (r[m == 0] == 1).all()


# ------------------------------------------------------------------------------------------------ losses
def _soft(rng, shape, hi=1.0):
    return rng.uniform(0, hi, shape).astype(f32)


@pytest.mark.parametrize("N,B,H", [(3, 3, 17), (4, 2, 8)])
def test_fused_losses_equal_the_oracles_on_half_representable_references(N, B, H):
    rng = np.random.default_rng(N)
    m = _soft(rng, (N, H, H))
    gt, edt = M.h(_soft(rng, (B, H, H))), M.h(_soft(rng, (B, H, H), 4.0))
    got = M.fused_sil_losses(m, gt, edt)
    tm = torch.from_numpy(m).double()
    tg, te = (torch.from_numpy(np.tile(x, (N // B, 1, 1))).double() for x in (gt, edt))
    m2, g2 = tm.reshape(N, -1), tg.reshape(N, -1)
    want = torch.stack([O.l1_loss(tm, tg, reduce=False), (m2 * g2).sum(1), (m2 + g2 - m2 * g2).sum(1),
                        O.edt_loss(tm, te[:, None], reduce=False)], 1).numpy()
    assert got.dtype == np.float64 and got.shape == (N, 4)
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=0)
    # and IoU through the oracle's own function: sum m g / (sum(m + g - m g) + eps)
    np.testing.assert_allclose(got[:, 1] / (got[:, 2] + 1e-6), O.iou(tm, tg, reduce=False).numpy(), rtol=1e-13)


@pytest.mark.parametrize("N,B,H", [(3, 3, 17), (4, 2, 8)])
def test_fused_grad_mask_is_the_gradient_of_the_fused_losses(N, B, H):
    """float64 autograd of sum(go * losses) at the half mask against the kernel's float32 expression: 1e-6 of scale."""
    rng = np.random.default_rng(10 + N)
    m_h = M.h(_soft(rng, (N, H, H)))
    gt, edt = M.h(_soft(rng, (B, H, H))), M.h(_soft(rng, (B, H, H), 4.0))
    go = rng.standard_normal((N, 4)).astype(f32)
    tm = torch.from_numpy(m_h).double().requires_grad_(True)
    tg, te = (torch.from_numpy(np.tile(x, (N // B, 1, 1))).double().reshape(N, -1) for x in (gt, edt))
    m2 = tm.reshape(N, -1)
    los = torch.stack([(m2 - tg).abs().mean(1), (m2 * tg).sum(1), (m2 + tg - m2 * tg).sum(1), (te * m2).mean(1)], 1)
    (los * torch.from_numpy(go).double()).sum().backward()
    got = M.fused_grad_mask(m_h, gt, edt, go)
    assert got.dtype == f32 and got.shape == (N, H, H)
    np.testing.assert_allclose(got, tm.grad.numpy(), rtol=0, atol=1e-6 * np.abs(tm.grad.numpy()).max())


@pytest.mark.parametrize("N,B,H", [(3, 3, 5), (4, 2, 8)])
def test_texture_mse_model(N, B, H):
    """The loss against oracle.masked_texture_mse; the gradient against float64 autograd AT THE STORED image; the scatter
    sum against oracle.tex_render_backward_atlas, shared atlases summed over their hypotheses."""
    rng = np.random.default_rng(20 + N)
    v = _soft(rng, (N, 3, H, H))
    ref, mk = M.h(_soft(rng, (B, 3, H, H))), M.h(_soft(rng, (B, H, H)))
    go = rng.standard_normal(N).astype(f32)
    G = N // B
    tref, tmk = torch.from_numpy(np.tile(ref, (G, 1, 1, 1))).double(), torch.from_numpy(np.tile(mk, (G, 1, 1))).double()
    want = O.masked_texture_mse(torch.from_numpy(v).double(), tref, tmk).numpy()
    np.testing.assert_allclose(M.tex_mse_loss(v, ref, mk), want, rtol=1e-13)
    x = torch.from_numpy(M.h(v)).double().requires_grad_(True)
    (O.masked_texture_mse(x, tref, tmk) * torch.from_numpy(go).double()).sum().backward()
    g = M.tex_mse_grad(M.h(v), ref, mk, go)
    assert g.dtype == f32
    np.testing.assert_allclose(g, x.grad.numpy(), rtol=0, atol=1e-6 * np.abs(x.grad.numpy()).max())
    F, R = 3, 2
    local = rng.integers(-1, F * R * R, (N, H, H))                      # (-1: the pixel shows no face)
    tidx = np.where(local >= 0, np.arange(N)[:, None, None] * F * R * R + local, -1).astype(np.int32)
    full = O.tex_render_backward_atlas(tidx, g, (N, F, R, R, 3))
    got = M.scatter_texels(g, M.shared_tidx(tidx, B, F * R * R), (B, F, R, R, 3))
    np.testing.assert_allclose(got, full.reshape(G, B, F, R, R, 3).astype(np.float64).sum(0), rtol=0,
                               atol=1e-6 * np.abs(full).max())
    assert np.array_equal(M.shared_tidx(tidx, N, F * R * R), tidx)


# ------------------------------------------------------------------------------------------------ the GPU test's inputs
_SEEN = {}


def _oracle(sc, K):
    key = (sc["name"], sc["H"], K)
    if key not in _SEEN:
        verts, cams = S.sil_inputs(sc)
        m32, _ = O.sil_render(verts, sc["faces"], cams, sc["H"], K=K)
        _SEEN[key] = (verts, cams, m32)
    return _SEEN[key]


def test_the_backward_scenes_bite():
    """On the oracle's masks of the scenes of test_backward_with_a_given_gradient: pixels with 0 < m32 < 1 whose
    r = (1 - m_h) / (1 - m32) is more than 1e-2 from 1, and pixels with m_h == 1 and m32 < 1 (r = 0: the half build
    sends no gradient through them, the fp32 build does).  Every mask is 0 in half exactly where it is 0 in float."""
    both, names = 0, set()
    for K in BWD_KS:
        for name, sc in backward_scenes(K):
            _, _, m32 = _oracle(sc, K)
            assert M.zero_mask_agrees(m32), (sc["name"], K)
            r = M.ratio(m32, M.h(m32))
            off = int(((m32 > 0) & (m32 < 1) & (np.abs(r - 1) > 1e-2)).sum())
            lost = int(((M.h(m32) == 1) & (m32 < 1)).sum())
            print("K=%2d %-30s H=%2d: %4d soft pixels, %3d with |r - 1| > 1e-2, %3d with m_h == 1 > m32" % (
                K, sc["name"], sc["H"], ((m32 > 0) & (m32 < 1)).sum(), off, lost))
            both += off > 0 and lost > 0
            if off > 0 and lost > 0:
                names.add((name, K))
    assert both > 0
    assert all((TEETH, K) in names for K in BWD_KS)                     # the scene whose teeth the GPU test asserts


@pytest.mark.parametrize("K", BWD_KS)
def test_the_two_readings_of_the_mask_differ_by_far_more_than_the_bar(K):
    """The oracle's backward of the TEETH scene, fed g and g r: relative L2 apart by more than 100 times the 1e-5 bar of
    the GPU comparison (which asserts 10 times on the kernels), for vertices and cameras."""
    (sc,) = [s for name, s in backward_scenes(K) if name == TEETH]
    verts, cams, m32 = _oracle(sc, K)
    g = upstream(sc, K)
    r = M.ratio(m32, M.h(m32))
    a = O.sil_render_backward(verts, sc["faces"], cams, sc["H"], g, K=K)
    b = O.sil_render_backward(verts, sc["faces"], cams, sc["H"], g * r, K=K)
    for x, y, what in ((a[0], b[0], "vertices"), (a[1], b[1], "cameras")):
        rel = np.linalg.norm(x.astype(np.float64) - y) / np.linalg.norm(x.astype(np.float64))
        print("%s K=%d %s: relative L2 between the two readings %.3g" % (sc["name"], K, what, rel))
        assert rel > 1e-3
