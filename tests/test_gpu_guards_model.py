"""GPU: the model-side units -- deformation (csrc/acfm_deform.hip, acfm_solve.hip), cameras (acfm_camera.hip) and
keypoints (acfm_keypoints.hip) -- on hostile, fenced memory: tests/guards.py run_case.

Bits everywhere but two places.  deform_apply's backward adds the handle and mean gradients with float atomics (no
deterministic mode): they are held to the float64 evaluation and the bars of test_deform_apply_wide in every run; its
gradient to P is a double sum rounded once and is bits.  camera_pipeline_tables' backward adds table rows with float
atomics: the frame ids of the case are distinct, so every row gets one addend and the result is bits."""
import numpy as np
import pytest
import torch

import guards
from test_gpu_deform_solve_wide import SMALL_CASES, _assert_small, _small_case
from test_gpu_keypoints import IMG, SHAPES, _cams, _gen, make_gt

pytestmark = pytest.mark.gpu
_report = guards.module_report(__name__)


def _d():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _leaf(t, d, grad=True):
    return t.clone().to(d).requires_grad_(grad)


# ------------------------------------------------------------------------------------------------ deformation
def test_deform_apply():
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    N, Kh, V = 3, 33, 50
    torch.manual_seed(N)
    mean, P, delta = torch.randn(V, 3), torch.randn(V, Kh), 0.1 * torch.randn(N, Kh, 3)
    w = torch.randn(N, V, 3)
    b = [t.clone().double().requires_grad_(True) for t in (mean, P, delta)]
    ref = b[0][None] + torch.matmul(b[1][None], b[2])
    (ref * w.double()).sum().backward()

    def fn(inp):
        a = [inp(_leaf(t, d)) for t in (mean, P, delta)]
        out = ops.deform_apply(*a)
        gm, gp, gd = torch.autograd.grad(out, a, inp(w.to(d)))
        np.testing.assert_allclose(out.detach().cpu().numpy(), ref.detach().numpy(), rtol=1e-5, atol=1e-5)
        for got, want in zip((gm, gp, gd), b):
            np.testing.assert_allclose(got.cpu().numpy(), want.grad.numpy(), rtol=1e-4, atol=1e-4)
        return dict(out=out, gm=gm, gp=gp, gd=gd)
    guards.run_case(fn, loose=("gm", "gd"))


@pytest.mark.parametrize("V,Kh", [min(SMALL_CASES, key=lambda c: c[0] * c[1]), (50, 33), (70, 65)])
def test_deform_solve(V, Kh):
    """deform_solve and its backward at the smallest SMALL_CASES entry, at 33 handles (a second panel of one column)
    and at 65; the workspace (factor, right-hand-side tiles with their self-validating words, the status word) is
    poisoned with both patterns."""
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    Lr, logits, ref, gref = _small_case(V, Kh)

    def fn(inp):
        lg = inp(_leaf(logits, d))
        P = ops.deform_solve(inp(Lr.to(d)), lg, check=True)
        g, = torch.autograd.grad(P.square().sum(), lg)
        _assert_small(P, ref)
        return dict(P=P, g=g)
    plain, _ = guards.run_case(fn)
    np.testing.assert_allclose(plain["g"].cpu().numpy(), gref.numpy(), rtol=1e-3, atol=1e-5 * float(gref.abs().max()))


# ------------------------------------------------------------------------------------------------ cameras
def _camera_rows(R, seed):
    g = _gen(seed)
    emb = torch.randn(R, 7, generator=g)
    emb[:, 3:] = torch.nn.functional.normalize(emb[:, 3:], dim=1)
    return emb


def test_camera_pipeline_mirror_normalize():
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    G, N = 3, 43
    R = G * N                                                  # 129 rows: past two waves by one
    emb = _camera_rows(R, 1)
    g = _gen(2)
    flag = torch.randint(0, 2, (N,), generator=g)
    tr = torch.cat([0.8 + 0.4 * torch.rand(N, 1, generator=g), 0.1 * torch.randn(N, 3, generator=g)], 1)
    w = torch.randn(R, 7, generator=g)

    def fn(inp):
        e = inp(_leaf(emb.reshape(G, N, 7), d))
        cams = ops.camera_pipeline(e, flag.to(d), inp(tr.to(d)), 0.05)
        ge, = torch.autograd.grad(cams, e, inp(w.to(d)))
        raw = inp(_leaf(emb, d))
        nrm = ops.camera_normalize(raw)
        gr, = torch.autograd.grad(nrm, raw, inp(w.to(d)))
        return dict(cams=cams, ge=ge, mirror=ops.camera_mirror(cams.detach()), nrm=nrm, gr=gr)
    guards.run_case(fn)


def test_camera_pipeline_tables():
    """A row whose frame id is outside the tables is a NaN camera by contract -- yet written: completeness holds, and
    the NaN row is the same bits in every run (a quiet NaN the kernel forms itself, not the poison)."""
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    G, N, F = 3, 43, 50
    tables = [_camera_rows(F, 10 + g) for g in range(G)]
    g = _gen(3)
    idx = torch.randperm(F, generator=g)[:N]                   # distinct frames: one addend per table row
    idx[7] = F + 5                                             # out of range
    flag = torch.randint(0, 2, (N,), generator=g)
    tr = torch.cat([0.8 + 0.4 * torch.rand(N, 1, generator=g), 0.1 * torch.randn(N, 3, generator=g)], 1)
    w = torch.randn(G * N, 7, generator=g)

    def fn(inp):
        ts = [inp(_leaf(t, d)) for t in tables]
        cams = ops.camera_pipeline_tables(ts, idx.to(d), flag.to(d), inp(tr.to(d)), 0.05)
        gs = torch.autograd.grad(cams, ts, inp(w.to(d)))
        return dict(cams=cams, **{"g%d" % i: t for i, t in enumerate(gs)})
    plain, _ = guards.run_case(fn)
    cams = plain["cams"].reshape(G, N, 7)
    assert bool(torch.isnan(cams[:, 7]).all()) and not bool(torch.isnan(cams[:, :7]).any()) \
        and not bool(torch.isnan(cams[:, 8:]).any())
    for i in range(G):
        assert not bool(torch.isnan(plain["g%d" % i]).any())


# ------------------------------------------------------------------------------------------------ keypoints
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2]], ids=str)
def test_keypoint_head(shape):
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    K, V, Nv, G, Ng = shape
    N = Nv * G
    g = _gen(200 + K)
    logits = 3 * torch.randn(K, V, generator=g)
    verts = 0.5 * torch.randn(Nv, V, 3, generator=g)
    cams = _cams(N, g)
    gt = make_gt(logits, verts, cams, Ng, g)
    w = dict(gA=torch.randn(K, V, generator=g), ge=torch.randn((), generator=g), gl=torch.randn(N, generator=g),
             gp=torch.randn(N, K, 2, generator=g), gv=torch.randn(Nv, K, 3, generator=g))

    def fn(inp):
        x, v, c = inp(_leaf(logits, d)), inp(_leaf(verts, d)), inp(_leaf(cams, d))
        A, ent = ops.kp_weights(x)
        kpv, kpp, loss, err = ops.kp_head(A, v, c, inp(gt.to(d)), IMG, True)
        obj = (loss * w["gl"].to(d)).sum() + (kpp * w["gp"].to(d)).sum() + (kpv * w["gv"].to(d)).sum() \
            + ent * w["ge"].to(d) + (A * w["gA"].to(d)).sum()
        gx, gv, gc = torch.autograd.grad(obj, (x, v, c))
        return dict(A=A, ent=ent, kpv=kpv, kpp=kpp, loss=loss, err=err, gx=gx, gv=gv, gc=gc)
    guards.run_case(fn)


@pytest.mark.parametrize("N,G", [(1, 0), (5, 0), (5, 3)])
def test_camera_loss(N, G):
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    g = _gen(300 + N + G)
    pred = _cams(N, g)
    ref = _cams(N, g)
    cams = _cams(max(G, 1) * N, g)
    probs = torch.rand(max(G, 1), N, generator=g)

    def fn(inp):
        p = inp(_leaf(pred, d))
        if G:
            loss, best = ops.camera_loss(p, margin=0.1, cams=inp(cams.to(d)), probs=inp(probs.to(d)))
        else:
            loss, best = ops.camera_loss(p, inp(ref.to(d)), margin=0.1)
        gp, = torch.autograd.grad(loss, p)
        return dict(loss=loss, best=best, gp=gp)
    guards.run_case(fn)
