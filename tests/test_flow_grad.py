"""CPU: the opt-in switch of the flow operators' backward (flow_ops.set_trainable / trainable), correlation_torch against
the oracle, and the helpers test_gpu_flow_grad.py shares: offsets nudged away from integer sample coordinates (the offset
gradient jumps there), the float64 autograd references, and a float64 closed form of the offset gradient that takes the
floor cell at an integer coordinate -- checked here against autograd where both are defined."""
import functools
import os
import re
import threading

import numpy as np
import torch

from conftest import ROOT
from oracle import oracle as O
from test_flow_ops import GPU_CASES, HOST_CASES, TOL, make_inputs

BOUND = 1e-4          # the project's gradient parity bound: max|got - ref| <= 1e-4 max|ref|


def _coords(off, H, W):
    """float64 sample coordinates [N, 9, 2, H, W] (row, column) of the nine taps for an 18- or a 2-channel offset."""
    off = np.asarray(off, np.float64)
    N = off.shape[0]
    ys, xs = np.mgrid[0:H, 0:W]
    c = np.empty((N, 9, 2, H, W))
    for t in range(9):
        ky, kx = divmod(t, 3)
        oh, ow = (off[:, 0], off[:, 1]) if off.shape[1] == 2 else (off[:, 2 * t], off[:, 2 * t + 1])
        c[:, t, 0], c[:, t, 1] = ys + ky - 1 + oh, xs + kx - 1 + ow
    return c


def min_integer_distance(off, H, W):
    c = _coords(off, H, W)
    return float(np.abs(c - np.rint(c)).min())


def nudge(off, H, W):
    """A float32 COPY of `off` in which every offset whose coordinate y+ky-1+off or x+kx-1+off lies within 1e-3 of an
    integer is moved by 2e-3 (again, if rounding to float32 brought it back); asserts the condition on the result."""
    off = np.array(off, np.float32, copy=True)
    shared = off.shape[1] == 2
    for _ in range(4):
        c = _coords(off, H, W)
        near = np.abs(c - np.rint(c)) < 1e-3                 # [N, 9, 2, H, W]
        if not near.any():
            break
        if shared:
            off = (off.astype(np.float64) + 2e-3 * near.any(1)).astype(np.float32)
        else:
            off = (off.astype(np.float64) + 2e-3 * near.reshape(off.shape)).astype(np.float32)
    assert min_integer_distance(off, H, W) >= 1e-3
    return off


def draw_go(shape, seed=11):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def dconv_ref_grads(x, off, w, b, go):
    """float64 autograd on the CPU of flow_ops.deform_conv2d_torch -> (gx, goff, gw, gb) as numpy float64."""
    from acfm_video_3d_reconstruction_amd.flow_ops import deform_conv2d_torch
    t = [torch.tensor(np.asarray(a), dtype=torch.float64, requires_grad=True) for a in (x, off, w, b)]
    out = deform_conv2d_torch(*t)
    return tuple(g.numpy() for g in torch.autograd.grad(out, t, torch.tensor(np.asarray(go), dtype=torch.float64)))


def corr_ref_grads(f1, f2, md, go):
    from acfm_video_3d_reconstruction_amd.correlation import correlation_torch
    t = [torch.tensor(np.asarray(a), dtype=torch.float64, requires_grad=True) for a in (f1, f2)]
    out = correlation_torch(t[0], t[1], md)
    return tuple(g.numpy() for g in torch.autograd.grad(out, t, torch.tensor(np.asarray(go), dtype=torch.float64)))


def offset_grad_closed_form(x, off, w, go):
    """float64 numpy: grad_offset[n, 2t] = sum_ci gcol[n,ci,t,p] dS/dh, [n, 2t+1] the same with dS/dw, where
    gcol = sum_co W[co,ci,t] go[n,co,p], dS/dh = uw (v10 - v00) + lw (v11 - v01), dS/dw = uh (v01 - v00) + lh (v11 - v10)
    on the FLOOR cell (lh = h - floor(h), 0 at an integer coordinate: the forward difference towards the +1 neighbour),
    corners outside the map counting 0 and the gradient 0 for a position outside (-1, H) x (-1, W).  A 2-channel offset
    gets the sum over the nine taps."""
    x, off, w, go = (np.asarray(a, np.float64) for a in (x, off, w, go))
    N, C, H, W = x.shape
    shared = off.shape[1] == 2
    c = _coords(off, H, W)
    gcol = np.einsum("oct,nohw->ncthw", w.reshape(w.shape[0], C, 9), go)
    g18 = np.zeros((N, 18, H, W))
    for n in range(N):
        for t in range(9):
            h, ww = c[n, t, 0], c[n, t, 1]
            inside = (h > -1) & (h < H) & (ww > -1) & (ww < W)
            h0, w0 = np.floor(h), np.floor(ww)
            lh, lw = h - h0, ww - w0
            uh, uw = 1.0 - lh, 1.0 - lw

            def corner(dh, dw):
                hi, wi = h0 + dh, w0 + dw
                ok = inside & (hi >= 0) & (hi <= H - 1) & (wi >= 0) & (wi <= W - 1)
                v = x[n][:, np.clip(hi, 0, H - 1).astype(np.int64), np.clip(wi, 0, W - 1).astype(np.int64)]
                return np.where(ok[None], v, 0.0)
            v00, v01, v10, v11 = corner(0, 0), corner(0, 1), corner(1, 0), corner(1, 1)
            g18[n, 2 * t] = (gcol[n, :, t] * (uw * (v10 - v00) + lw * (v11 - v01))).sum(0)
            g18[n, 2 * t + 1] = (gcol[n, :, t] * (uh * (v01 - v00) + lh * (v11 - v10))).sum(0)
    return np.stack((g18[:, 0::2].sum(1), g18[:, 1::2].sum(1)), 1) if shared else g18


def ratio(got, ref):
    """max|got - ref| / max|ref| (a reference of all zeros asks for exact zeros: the ratio is then 0 or inf)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err, top = float(np.abs(got - ref).max()), float(np.abs(ref).max())
    return err / top if top > 0 else (0.0 if err == 0 else float("inf"))


# ---------------------------------------------------------------------------------------------------- the switch
def test_switch_is_off_by_default_and_restores():
    from acfm_video_3d_reconstruction_amd import flow_ops
    assert flow_ops.is_trainable() is False
    assert flow_ops.set_trainable(True) is False
    assert flow_ops.is_trainable() is True
    assert flow_ops.set_trainable(False) is True
    with flow_ops.trainable():
        assert flow_ops.is_trainable()
        with flow_ops.trainable(False):
            assert not flow_ops.is_trainable()
        assert flow_ops.is_trainable()
    assert not flow_ops.is_trainable()
    try:
        with flow_ops.trainable():
            raise KeyError("x")
    except KeyError:
        pass
    assert not flow_ops.is_trainable()


def test_switch_is_process_wide():
    from acfm_video_3d_reconstruction_amd import flow_ops
    seen = []
    with flow_ops.trainable():
        th = threading.Thread(target=lambda: seen.append(flow_ops.is_trainable()))
        th.start()
        th.join()
    th = threading.Thread(target=lambda: seen.append(flow_ops.is_trainable()))
    th.start()
    th.join()
    assert seen == [True, False]


def test_host_tensors_do_not_depend_on_the_switch():
    from acfm_video_3d_reconstruction_amd import flow_ops
    x, o18, _, w, b = make_inputs(*HOST_CASES[0])
    m = flow_ops.DeformConv2d(5, 3, 3, padding=1)
    with torch.no_grad():
        ref = m(torch.tensor(x), torch.tensor(o18))
    with flow_ops.trainable():
        out = m(torch.tensor(x), torch.tensor(o18))
        assert out.requires_grad and torch.equal(out.detach(), ref)


# ---------------------------------------------------------------------------------------------------- definitions
def test_correlation_torch_equals_the_oracle():
    from acfm_video_3d_reconstruction_amd.correlation import correlation_torch
    rng = np.random.default_rng(5)
    for (N, C, H, W, md) in ((2, 5, 7, 9, 1), (1, 19, 17, 33, 4), (1, 3, 1, 1, 3), (2, 16, 6, 12, 2)):
        f1 = rng.standard_normal((N, C, H, W)).astype(np.float32)
        f2 = rng.standard_normal((N, C, H, W)).astype(np.float32)
        ref = O.correlation(f1, f2, md)
        got64 = correlation_torch(torch.tensor(f1).double(), torch.tensor(f2).double(), md)
        got32 = correlation_torch(torch.tensor(f1), torch.tensor(f2), md)
        assert got64.shape == ref.shape and got32.dtype == torch.float32
        np.testing.assert_allclose(got64.numpy(), ref, **TOL)
        np.testing.assert_allclose(got32.numpy(), ref, **TOL)
    t1 = torch.tensor(f1, requires_grad=True)
    correlation_torch(t1, torch.tensor(f2), md).sum().backward()
    assert t1.grad is not None


def test_nudge_leaves_the_cached_arrays_alone():
    case = GPU_CASES[1]
    o18 = make_inputs(*case)[1]
    before = o18.copy()
    n18 = nudge(o18, case[3], case[4])
    assert np.array_equal(o18, before) and n18 is not o18
    assert min_integer_distance(n18, case[3], case[4]) >= 1e-3
    assert np.abs(n18 - o18).max() <= 4.1e-3


def test_closed_form_offset_gradient_equals_float64_autograd():
    """The helper that pins the integer-coordinate convention on the GPU, checked where autograd defines the gradient:
    nudged (non-integer) offsets, both offset forms, one case with most taps outside."""
    for case in (HOST_CASES[0], (1, 3, 4, 7, 9, 8.0)):
        N, Cin, Cout, H, W, _ = case
        x, o18, o2, w, b = make_inputs(*case)
        go = draw_go((N, Cout, H, W))
        for off in (nudge(o18, H, W), nudge(o2, H, W)):
            ref = dconv_ref_grads(x, off, w, b, go)[1]
            got = offset_grad_closed_form(x, off, w, go)
            assert float(np.abs(ref).max()) > 0
            np.testing.assert_allclose(got, ref, rtol=0, atol=1e-9)


def test_new_symbols_are_declared():
    txt = open(os.path.join(ROOT, "include", "acfm_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("acfm_correlation_backward", "acfm_deform_conv2d_backward", "acfm_deform_conv2d_backward_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, txt), name
    from acfm_video_3d_reconstruction_amd import _lib
    h = _lib.lib()
    assert h.acfm_deform_conv2d_backward_workspace_bytes(1, 196, 6, 12, 196) >= 4 * 196 * 196 * 9
    assert h.acfm_deform_conv2d_backward_workspace_bytes(0, 196, 6, 12, 196) == 0
    # NULL pointers and sizes out of range are refused before anything is launched (no GPU is needed for that)
    assert h.acfm_correlation_backward(None, None, None, 1, 4, 4, 4, 2, None, None, None) == 1
    assert h.acfm_deform_conv2d_backward(None, None, None, None, 1, 4, 4, 4, 4, 0, None, None, None, None, None, 0, None) == 1
