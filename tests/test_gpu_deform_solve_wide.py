"""GPU: the deformation solve with more than 32 handles (csrc/acfm_solve.hip: ceil(K_h / 32) panels of right-hand
sides in the single launch, up to 128 handles) -- the reference's 64-handle bird model and its 128-handle default.
Bounds and constructions are those of test_gpu_losses.py::test_deform_solve_native; the references are fp64 torch
evaluations of the reference's expression, made once per case."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle import oracle as O

pytestmark = pytest.mark.gpu

MESH_CASES = [("bird", 64), ("bird", 33), ("horse", 48), ("cow", 128), ("horse", 100)]
# one handle into the second panel; three panels, the last nearly empty, three matrix tiles; Kh > V with two tiles;
# exact multiples; four full panels with Kh > n_pad; one matrix tile with two panels
SMALL_CASES = [(50, 33), (70, 65), (33, 64), (96, 96), (40, 128), (5, 34)]


def _d():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _ref(L, logits, loss):
    """fp64: P = (L^T L + A^T A)^-1 A^T and d loss(P) / d logits."""
    l64 = logits.double().requires_grad_(True)
    A = torch.softmax(l64, dim=0).t()
    M = L.double().t() @ L.double() + A.t() @ A
    ref = torch.cholesky_solve(A.t(), torch.linalg.cholesky(M))
    loss(ref).backward()
    return ref.detach(), l64.grad


@functools.lru_cache(maxsize=None)
def _mesh_case(name, Kh):
    from acfm_video_3d_reconstruction_amd.synthetic import fps_lbs_logits
    m = np.load(os.path.join(GOLDEN, "meshes.npz"))
    v, f = torch.from_numpy(m[name + "_v"]), torch.from_numpy(m[name + "_f"])
    L = O.laplacian_cot(v.double(), f).float()
    logits = torch.tensor(fps_lbs_logits(v.numpy(), Kh))
    torch.manual_seed(Kh)
    w = torch.randn(v.shape[0], Kh)
    ref, gref = _ref(L, logits, lambda P: (P * w.double()).sum())
    return L, logits, w, ref, gref


@functools.lru_cache(maxsize=None)
def _small_case(V, Kh, logits_seed=None):
    """Random L of seed V; logits of the same stream, or of a seed of their own."""
    torch.manual_seed(V)
    Lr = torch.randn(V, V)
    logits = torch.randn(V, Kh)
    if logits_seed is not None:
        logits = torch.randn(V, Kh, generator=torch.Generator().manual_seed(logits_seed))
    ref, gref = _ref(Lr, logits, lambda P: P.square().sum())
    return Lr, logits, ref, gref


def _assert_small(P, ref):
    np.testing.assert_allclose(P.detach().cpu().numpy(), ref.numpy(), rtol=1e-4, atol=1e-6 * float(ref.abs().max()))


@pytest.mark.parametrize("name,Kh", MESH_CASES)
def test_wide_solve_on_meshes(name, Kh):
    """Real meshes against the fp64 expression of the reference, P and the lbs gradient."""
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    L, logits, w, ref, gref = _mesh_case(name, Kh)
    lg = logits.clone().to(d).requires_grad_(True)
    P = ops.deform_solve(L.to(d), lg, check=True)
    (P * w.to(d)).sum().backward()
    eP = float((P.detach().cpu().double() - ref).abs().max()) / float(ref.abs().max())
    eg = float((lg.grad.cpu().double() - gref).abs().max()) / float(gref.abs().max())
    print("%s/%d: |P - ref| / max|ref| = %.2e, |g - ref| / max|g| = %.2e" % (name, Kh, eP, eg))
    assert eP < 1e-5, (name, Kh)
    assert eg < 1e-4, (name, Kh)


@pytest.mark.parametrize("V,Kh", SMALL_CASES)
def test_wide_solve_panel_edges(V, Kh):
    """The smallest shapes at which every panel edge occurs, random L."""
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    Lr, logits, ref, gref = _small_case(V, Kh)
    lg = logits.clone().to(d).requires_grad_(True)
    P = ops.deform_solve(Lr.to(d), lg, check=True)
    P.square().sum().backward()
    print("(%d, %d): max |P - ref| = %.2e of %.2e, max |g - ref| = %.2e of %.2e" % (
        V, Kh, float((P.detach().cpu().double() - ref).abs().max()), float(ref.abs().max()),
        float((lg.grad.cpu().double() - gref).abs().max()), float(gref.abs().max())))
    _assert_small(P, ref)
    np.testing.assert_allclose(lg.grad.cpu().numpy(), gref.numpy(), rtol=1e-3, atol=1e-5 * float(gref.abs().max()))


def test_wide_solve_reused_workspace():
    """Two calls of the C entry point in ONE workspace with different logits: the second answers for its own input.
    Every right-hand-side tile row is published through self-validating words, so every one has to be poisoned again;
    a row left out hands the first call's Y^T to the second call's P = R Y."""
    from acfm_video_3d_reconstruction_amd import _lib
    d = _d()
    V, Kh = 70, 65
    Lr, logits_a, ref_a, _ = _small_case(V, Kh)
    _, logits_b, ref_b, _ = _small_case(V, Kh, logits_seed=1000 + V)
    assert float((ref_a - ref_b).abs().max()) > 1e-3 * float(ref_b.abs().max())  # the two answers do differ
    nbytes = _lib.lib().acfm_deform_solve_workspace_bytes(V, Kh)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=d)
    l = Lr.to(d).contiguous()
    for logits, ref in ((logits_a, ref_a), (logits_b, ref_b)):
        b = logits.to(d).contiguous()
        P = torch.empty((V, Kh), dtype=torch.float32, device=d)
        _lib.call("acfm_deform_solve", d, _lib.ptr(l), _lib.ptr(b), V, Kh, _lib.ptr(P), _lib.ptr(ws), nbytes)
        info = ctypes.c_int(-1)
        _lib.call("acfm_deform_solve_info", d, _lib.ptr(ws), nbytes, V, ctypes.byref(info))
        assert info.value == 0
        _assert_small(P, ref)


def test_wide_solve_repeats_and_graph_replay():
    """64 handles on the horse: repeated solves give equal bits, and so does a captured graph (the sentinel fill of all
    the right-hand-side tile rows is part of the captured sequence)."""
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    L, logits, _, ref, _ = _mesh_case("horse", 64)
    Lh, lh = L.to(d), logits.to(d)
    first = ops.deform_solve(Lh, lh, check=True).clone()
    assert float((first.cpu().double() - ref).abs().max()) < 1e-5 * float(ref.abs().max())
    for _ in range(5):
        assert torch.equal(ops.deform_solve(Lh, lh), first)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        out = ops.deform_solve(Lh, lh)  # warm-up on the capture stream
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            out = ops.deform_solve(Lh, lh)
    for _ in range(3):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, first)


@pytest.mark.parametrize("N,Kh,V", [(3, 33, 50), (5, 64, 642), (2, 128, 70)])
def test_deform_apply_wide(N, Kh, V):
    """verts = mean + P delta and its backward with more than 32 handles, vs an fp64 evaluation (the kernels of
    csrc/acfm_deform.hip were general in K_h already: this pins the ground the wider solve feeds)."""
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    torch.manual_seed(N)
    mean, P, delta = torch.randn(V, 3), torch.randn(V, Kh), 0.1 * torch.randn(N, Kh, 3)
    w = torch.randn(N, V, 3)
    a = [t.clone().to(d).requires_grad_(True) for t in (mean, P, delta)]
    out = ops.deform_apply(*a)
    (out * w.to(d)).sum().backward()
    b = [t.clone().double().requires_grad_(True) for t in (mean, P, delta)]
    ref = b[0][None] + torch.matmul(b[1][None], b[2])
    (ref * w.double()).sum().backward()
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref.detach().numpy(), rtol=1e-5, atol=1e-5)
    for x, y in zip(a, b):
        np.testing.assert_allclose(x.grad.cpu().numpy(), y.grad.numpy(), rtol=1e-4, atol=1e-4)


def test_deform_solver_64_handles_end_to_end(meshes):
    """DeformSolver with the 64 handles of the reference's best bird model: output and the gradients to lbs and delta
    against the fp64 formula and its autograd."""
    from acfm_video_3d_reconstruction_amd.deform import DeformSolver
    from acfm_video_3d_reconstruction_amd.synthetic import fps_lbs_logits
    d = _d()
    v, f = torch.from_numpy(meshes["bird_v"]), torch.from_numpy(meshes["bird_f"])
    logits = torch.tensor(fps_lbs_logits(v.numpy(), 64))
    gen = torch.Generator().manual_seed(64)
    delta = 0.05 * torch.randn(4, 64, 3, generator=gen)
    w = torch.randn(4, v.shape[0], 3, generator=gen)
    L64 = O.laplacian_cot(v.double(), f)
    lr = logits.double().clone().requires_grad_(True)
    dr = delta.double().clone().requires_grad_(True)
    truth = O.deform_solve(lr, v, dr, L64)
    (truth * w.double()).sum().backward()
    lg = torch.nn.Parameter(logits.clone().to(d))
    solver = DeformSolver(v.to(d), f.to(d), lg)
    dl = delta.clone().to(d).requires_grad_(True)
    out = solver(dl)
    (out * w.to(d)).sum().backward()
    assert float((out.detach().cpu().double() - truth.detach()).abs().max()) < 1e-4
    np.testing.assert_allclose(dl.grad.cpu().numpy(), dr.grad.numpy(), rtol=1e-3, atol=1e-5)
    sc = np.abs(lr.grad.numpy()).max()
    np.testing.assert_allclose(lg.grad.cpu().numpy(), lr.grad.numpy(), rtol=1e-2, atol=1e-3 * sc)


def test_wide_solve_limits():
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    with pytest.raises(ValueError, match="at most 128 handles"):
        ops.deform_solve(torch.eye(140, device=d), torch.zeros(140, 129, device=d), check=True)
    # a matrix that is not positive definite is reported from the later panels' size too
    with pytest.raises(RuntimeError):
        ops.deform_solve(torch.zeros(40, 40, device=d), torch.full((40, 40), float("nan"), device=d), check=True)
