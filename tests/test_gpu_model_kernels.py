"""GPU: the three units at the head of every training step -- cameras (csrc/acfm_camera.hip), projection
(csrc/acfm_project.hip) and the deformation apply (csrc/acfm_deform.hip) -- against the float64 references of
tests/model_cases.py (pinned on the CPU by tests/test_model_cases.py) at the sizes where their code changes path:

  cameras     R = G N in {1, 127, 128, 129, 300} rows (128 rows per workgroup) with N that does not divide 128, both
              decays, all four (mirror, transform) flag combinations, relu on and off, q0 of both signs, a zero
              quaternion; the tables form with and without `selected`, a frame id that occurs twice, a `selected` that
              picks one table twice (both sum in the table gradient, as nn.Embedding does), a frozen table;
              camera_normalize / camera_mirror at quaternion norms 0, 1e-13, 1e-6, 1, 1e3
  projection  V in {1, 63, 64, 65, 192, 193, 255, 256, 257, 642, 2562} x N in {1, 3}, non-unit quaternions, both
              offsets, the backward with both inputs, the vertices only and the cameras only requiring grad
  deform      26 (N, Kh, V) that cover N in {1, 7, 11, 21, 22, 65, 130}, Kh in {1, 2, 3, 4, 5, 16, 17} and
              V in {1, 15, 16, 17, 64, 65, 642}; every subset of (mean, P, delta) requiring grad; the double sums handed
              to a presolve sink; the MFMA form of grad_P, which no Python path launches, through the C ABI

Bars: forward rtol 1e-6 / atol 1e-6 and gradients at the suite's bar (_close of test_gpu_loss_shapes.py: 1e-4 of the
reference's largest entry and 1e-5 relative L2) for the cameras and the projection's vertex gradient; the projection's
camera gradient against the float32 summation bound of model_cases.camera_grad_bound; the deformation apply at the bars
of test_deform_apply_wide (forward 1e-5, gradients 1e-4) and its d P within one ulp of the rounded float64 sum."""
import numpy as np
import pytest
import torch

import model_cases as M
from oracle import oracle as O
from test_gpu_loss_shapes import _close

pytestmark = pytest.mark.gpu

FWD = dict(rtol=1e-6, atol=1e-6)


def _d():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _np(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------ cameras
def _close_rows(got, ref, zero_row, what):
    """[R,7] gradients at the suite's bar; the zero-quaternion row apart (its quaternion part is 1/eps-scaled: as the
    scale of the whole tensor it would hide every other row)."""
    got, ref = got.detach().cpu().reshape(-1, 7), ref.reshape(-1, 7)
    keep = torch.ones(ref.shape[0], dtype=torch.bool)
    if zero_row is not None:
        keep[zero_row] = False
        _close(got[zero_row, :3], ref[zero_row, :3], what=what + " zero-q row, s t")
        _close(got[zero_row, 3:], ref[zero_row, 3:], what=what + " zero-q row, q")
        assert float(ref[zero_row, 3:].abs().max()) > 1e9
    _close(got[keep], ref[keep], what=what)


@pytest.mark.parametrize("G,N", M.CAMERA_SHAPES)
@pytest.mark.parametrize("decay", M.DECAYS)
def test_camera_pipeline(G, N, decay):
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    for variant in (range(4) if N == 1 else (0,)):
        c = M.camera_case(G, N, decay, variant)
        ref, gref = M.camera_ref(c["emb"], c["mirror"], c["tr"], decay, c["w"])
        e = c["emb"].to(d).requires_grad_(True)
        out = ops.camera_pipeline(e, c["mirror"].to(d), c["tr"].to(d), decay)
        ge, = torch.autograd.grad(out, e, c["w"].to(d))
        assert out.shape == (G * N, 7)
        np.testing.assert_allclose(_np(out), ref.numpy(), **FWD)
        _close_rows(ge, gref, c["rows"].get("zero_q"), "camera_pipeline %s" % ((G, N, decay, variant),))
        if c["rows"]:
            assert float(ge.reshape(-1, 7)[c["rows"]["relu_off"], 0]) == 0.0


@pytest.mark.parametrize("G,N,kind", M.TABLES_CASES)
def test_camera_pipeline_tables(G, N, kind):
    """The table gradient is a float-atomic sum; every cell of these cases collects at most two addends
    (model_cases.cell_addends), whose float32 sum does not depend on their order: a frozen table leaves the bits of the
    other tables' gradients alone."""
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    c = M.tables_case(G, N, kind)
    ref, grefs = M.tables_ref(c)
    fi, mf, tr, w = c["fi"].to(d), c["mirror"].to(d), c["tr"].to(d), c["w"].to(d)
    sel = None if c["sel"] is None else c["sel"].to(d)

    def run(frozen):
        ts = [t.to(d).requires_grad_(i != frozen) for i, t in enumerate(c["tables"])]
        out = ops.camera_pipeline_tables(ts, fi, mf, tr, 0.05, num_guesses=G, selected=sel)
        (out * w).sum().backward()
        return out.detach(), [t.grad for t in ts]
    out, gs = run(None)
    np.testing.assert_allclose(_np(out), ref.numpy(), **FWD)
    for t in range(c["T"]):
        _close(gs[t], grefs[t], what="table %d of %s" % (t, (G, N, kind)))
    read = int(c["sel"][0, 0]) if c["sel"] is not None else 0          # a table the batch does read
    assert M.cell_addends(c)[read].sum() > 0
    out2, gs2 = run(read)
    assert torch.equal(out2, out) and gs2[read] is None
    for t in range(c["T"]):
        if t != read:
            assert torch.equal(gs2[t], gs[t]), t


@pytest.mark.parametrize("R", [g * n for g, n in M.CAMERA_SHAPES])
def test_camera_normalize_and_mirror(R):
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    raw, w = M.raw_cameras(R)
    ref, gref = M.normalize_ref(raw, w)
    x = raw.to(d).requires_grad_(True)
    out = ops.camera_normalize(x)
    g, = torch.autograd.grad(out, x, w.to(d))
    np.testing.assert_allclose(_np(out), ref.numpy(), **FWD)
    for k, nrm in enumerate(M.QUAT_NORMS):                     # per norm: the gradients are 1 / max(|q|, 1e-12)-scaled
        if k < R:
            _close(g[k::5, 3:], gref[k::5, 3:], what="camera_normalize R %d |q| %g" % (R, nrm))
    assert torch.equal(g[:, :3].cpu(), w[:, :3])
    np.testing.assert_allclose(_np(ops.camera_mirror(raw.to(d))), M.mirror_ref(raw).numpy(), rtol=0, atol=0)
    np.testing.assert_allclose(_np(ops.camera_mirror(out.detach())), M.mirror_ref(out.detach().cpu()).numpy(), rtol=0,
                               atol=0)


# ------------------------------------------------------------------------------------------------ projection
def _project_run(fn, verts, cams, w, off, need_v, need_c):
    d = _d()
    v, c = verts.to(d).requires_grad_(need_v), cams.to(d).requires_grad_(need_c)
    out = fn(v, c, off)
    (out * w.to(d)).sum().backward()
    return out.detach(), v.grad, c.grad


@pytest.mark.parametrize("V", M.PROJECT_V)
@pytest.mark.parametrize("N", M.PROJECT_N)
def test_project(N, V):
    """Forward and backward of project and project_xy.  Bit equality of the three backward runs: a vertex's gradient
    is written by the thread that owns the vertex, and the camera gradient is summed in an order the kernel fixes
    (each thread adds its vertices v = tid, tid + 256, ... in turn, a butterfly over the wave, the four wave sums left
    to right) -- a null output pointer only skips stores, so freezing one input cannot move a bit of the other's."""
    from acfm_video_3d_reconstruction_amd import ops
    verts, cams, w = M.project_case(N, V)
    for off in M.PROJECT_OFFSETS:
        ref, gv_ref, gc_ref = M.project_ref(verts, cams, w, off)
        full = None
        for name, fn, ww in (("project", ops.project, w), ("project_xy", ops.project_xy, w[..., :2].contiguous())):
            xy = name == "project_xy"
            if xy:
                _, gv_ref, gc_ref = M.project_ref(verts, cams, w, off, xy=True)
            out, gv, gc = _project_run(fn, verts, cams, ww, off, True, True)
            want = ref[..., :2] if xy else ref
            assert out.shape == want.shape
            assert (np.abs(_np(out).astype(np.float64) - want.numpy())
                    <= M.project_forward_bound(verts, cams, off).numpy()).all()
            if xy:
                assert torch.equal(out, full[..., :2])
            else:
                full = out
                np.testing.assert_array_equal(_np(out), O.project(verts.numpy(), cams.numpy(), off))
            _close(gv, gv_ref, what="%s d verts %s" % (name, (N, V, off)))
            w3 = w.clone()
            if xy:
                w3[..., 2] = 0
            bound = M.camera_grad_bound(verts, cams, w3)
            err = np.abs(_np(gc).astype(np.float64) - gc_ref.numpy())
            print("%s N %d V %d offset %g: camera gradient max err %.3g, bound there %.3g, max err / bound %.3g" % (
                name, N, V, off, err.max(), bound.reshape(-1)[err.argmax()], (err / bound).max()))
            assert (err <= bound).all(), (name, N, V, off, float((err / bound).max()))
            out_v, gv_v, gc_v = _project_run(fn, verts, cams, ww, off, True, False)
            out_c, gv_c, gc_c = _project_run(fn, verts, cams, ww, off, False, True)
            assert gc_v is None and gv_c is None
            assert torch.equal(out_v, out) and torch.equal(out_c, out)
            assert torch.equal(gv_v, gv) and torch.equal(gc_c, gc)


# ------------------------------------------------------------------------------------------------ deformation apply
def _deform_run(N, Kh, V, needs=(True, True, True)):
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    m, p, dl, w = M.deform_case(N, Kh, V)
    a = [t.to(d).requires_grad_(n) for t, n in zip((m, p, dl), needs)]
    out = ops.deform_apply(*a)
    (out * w.to(d)).sum().backward()
    return out.detach(), [t.grad for t in a]


_JOINT = {}


def _joint(N, Kh, V):
    if (N, Kh, V) not in _JOINT:
        _JOINT[N, Kh, V] = _deform_run(N, Kh, V)
    return _JOINT[N, Kh, V]


@pytest.mark.parametrize("N,Kh,V", M.DEFORM_SHAPES)
def test_deform_apply(N, Kh, V):
    out, (gm, gp, gd) = _joint(N, Kh, V)
    ref, gm_ref, gp_ref, gd_ref = M.deform_ref(N, Kh, V)
    assert out.shape == (N, V, 3)
    np.testing.assert_allclose(_np(out), ref.numpy(), rtol=1e-5, atol=1e-5)
    for got, want in ((gm, gm_ref), (gp, gp_ref), (gd, gd_ref)):
        np.testing.assert_allclose(_np(got), want.numpy(), rtol=1e-4, atol=1e-4)
    # d P: a double sum rounded once, against the float64 sum rounded to float32
    _, p, dl, w = M.deform_case(N, Kh, V)
    G, _ = M.presolve_ref(dl, w)
    ulps = M.ulp_distance(_np(gp), G.astype(np.float32))
    print("(%d, %d, %d): %d of %d entries of d P one ulp from the rounded float64 sum" % (N, Kh, V, (ulps > 0).sum(),
                                                                                         ulps.size))
    assert ulps.max() <= 1


SUBSETS = [s for s in ((a, b, c) for a in (True, False) for b in (True, False) for c in (True, False)) if any(s)]


@pytest.mark.parametrize("N,Kh,V", M.DEFORM_SUBSET_SHAPES)
@pytest.mark.parametrize("needs", SUBSETS, ids=lambda s: "".join(n for n, on in zip("mPd", s) if on))
def test_deform_apply_subsets(N, Kh, V, needs):
    """Every subset of (mean, P, delta) requiring grad is another set of null pointers in k_deform_bwd_dm and another
    choice of launches.  d P (double sum, fixed order) and d mean / d delta (k_deform_bwd_dm: each wave's partial tile
    in v order, the 16 partial tiles summed left to right, no atomics) are the bits of the joint run."""
    out, grads = _joint(N, Kh, V)
    out_s, grads_s = _deform_run(N, Kh, V, needs)
    assert torch.equal(out_s, out)
    for name, on, got, want in zip(("mean", "P", "delta"), needs, grads_s, grads):
        if on:
            assert torch.equal(got, want), name
        else:
            assert got is None, name


class _Sink:
    def presolve_buffer(self, V, Kh, device):
        self.g64 = torch.full((V, Kh), float("nan"), dtype=torch.float64, device=device)
        self.m64 = torch.full((V, 3), float("nan"), dtype=torch.float64, device=device)
        return self.g64, self.m64


@pytest.mark.parametrize("N,Kh,V", [(65, 3, 17), (130, 5, 65)])
def test_deform_presolve_sink(N, Kh, V):
    """The doubles a registered sink receives (G = sum g delta^T and sum g: the second and third trip of the 64-frame
    stride, mean64 from the last quarter's wave, which at Kh = 3 owns no handle) against float64 numpy."""
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    m, p, dl, w = M.deform_case(N, Kh, V)
    G, sg = M.presolve_ref(dl, w)
    P = p.to(d).requires_grad_(True)
    sink = _Sink()
    key = ops.register_presolve_sink(P, sink)
    try:
        out = ops.deform_apply(m.to(d), P, dl.to(d))
        out.backward(w.to(d))
    finally:
        ops.drop_presolve_sink(key)
    g64, m64 = _np(sink.g64), _np(sink.m64)
    print("(%d, %d, %d): G64 max err %.3g of %.3g, mean64 max err %.3g of %.3g" % (
        N, Kh, V, np.abs(g64 - G).max(), np.abs(G).max(), np.abs(m64 - sg).max(), np.abs(sg).max()))
    assert np.abs(g64 - G).max() <= 1e-12 * np.abs(G).max()
    assert np.abs(m64 - sg).max() <= 1e-12 * np.abs(sg).max()
    assert torch.equal(P.grad, sink.g64.float())                # rounded once, from these doubles
    assert torch.equal(P.grad, _joint(N, Kh, V)[1][1])          # and the same bits without a sink


@pytest.mark.parametrize("N,Kh,V", M.DEFORM_GRAD_P_SHAPES)
def test_deform_grad_P_mfma(N, Kh, V):
    """acfm_deform_apply_backward with a non-null grad_P: k_deform_grad_P, the float32 MFMA form that
    include/acfm_hip.h documents and ops._DeformApply.backward never asks for."""
    from acfm_video_3d_reconstruction_amd import _lib
    d = _d()
    _, p, dl, w = M.deform_case(N, Kh, V)
    _, gm_ref, gp_ref, gd_ref = M.deform_ref(N, Kh, V)
    p, dl, w = p.to(d).contiguous(), dl.to(d).contiguous(), w.to(d).contiguous()
    nan = float("nan")
    gP, gd, gm = torch.full((V, Kh), nan, device=d), torch.full((N, Kh, 3), nan, device=d), torch.full((V, 3), nan, device=d)
    _lib.call("acfm_deform_apply_backward", d, _lib.ptr(p), _lib.ptr(dl), _lib.ptr(w), N, V, Kh, _lib.ptr(gd),
              _lib.ptr(gm), _lib.ptr(gP))
    for got, want in ((gm, gm_ref), (gP, gp_ref), (gd, gd_ref)):
        np.testing.assert_allclose(_np(got), want.numpy(), rtol=1e-4, atol=1e-4)
    only = torch.full((V, Kh), nan, device=d)
    _lib.call("acfm_deform_apply_backward", d, _lib.ptr(p), _lib.ptr(dl), _lib.ptr(w), N, V, Kh, None, None,
              _lib.ptr(only))
    assert torch.equal(only, gP)
