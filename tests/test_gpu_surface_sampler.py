"""GPU: the surface draw of csrc/acfm_sample.hip (k_surface_cdf, k_surface_sample, k_surface_bwd_lds /
k_surface_bwd_scatter) through ops.sample_surface and the shim, against surface_sampling.surface_sample_host -- the
definition, which tests/test_surface_sampler.py holds to its distribution on the host -- and the fit loop of
template_fit, eager and as a replayed hipGraph.

Forward: face ids and (u, v) equal the definition exactly; points within 1e-6 on unit-scale meshes (the library is
compiled without contraction and with correctly rounded division and sqrt, so they are expected to be equal too).
Backward: against float64 np.add.at.  A vertex's gradient component is a float32 sum, in any order, of n products
w g.  With u = 2^-24: the additions are off by at most (n - 1) u sum |w g| and the products by u |w g| each (first
order); the float32 weights themselves -- sqrt(u), 1 - su, su (1 - v), su v, all at most 1, 1 - v exact -- are within
2 u of the exact ones ABSOLUTELY, which adds 2 u |g| per term.  So per component
    |error| <= (n + 1) 2^-24 sum |w g| + 2 2^-24 sum |g|,
which _check_backward forms per vertex from the float64 terms; a row no sample touches must be exactly 0."""
import numpy as np
import pytest
import torch

import guards
from test_surface_sampler import TWO_F, TWO_V, blob, grad_reference, pack, weights64

pytestmark = pytest.mark.gpu
_report = guards.module_report(__name__)

SIZES_F = [1, 63, 64, 65, 257, 1025, 4100]      # one lane, the wave edge, one / two / five scan chunks with carry
SIZES_S = [1, 63, 64, 65, 1000]
BWD_LDS_MAX_V = 12800                           # SS_BWD_LDS_MAX_V of csrc/acfm_sample.hip


def _d():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _state(seed, draw, d):
    return torch.tensor([seed, draw], dtype=torch.int64, device=d)


def _run(state, vp, fp, first, S, d, vpm=0, faces_dtype=torch.int64, first_on_device=False):
    from acfm_video_3d_reconstruction_amd import ops
    tf = torch.from_numpy(fp).to(d).to(faces_dtype)
    t1 = torch.tensor(first, dtype=torch.int64)
    pts, fidx, uv = ops.sample_surface_uv(state, torch.tensor(vp, device=d), tf, t1.to(d) if first_on_device else t1, S, vpm)
    assert pts.dtype == torch.float32 and fidx.dtype == torch.int32 and uv.dtype == torch.float32
    return pts.cpu().numpy(), fidx.cpu().numpy(), uv.cpu().numpy()


def _check_forward(what, got, seed, draw, vp, fp, first, S):
    from acfm_video_3d_reconstruction_amd.surface_sampling import surface_sample_host
    pts, fidx, uv = got
    rp, rf, ruv = surface_sample_host(seed, draw, vp, fp, first, S)
    err = float(np.abs(pts.astype(np.float64) - rp).max())
    print("%s: %d of %d face ids differ, %d (u, v) differ, points max err %.2e (bar 1e-6), bit-equal %s"
          % (what, int((fidx != rf).sum()), fidx.size, int((uv != ruv).sum()), err, np.array_equal(pts, rp)))
    assert np.array_equal(fidx, rf), what
    assert np.array_equal(uv, ruv), what
    assert err <= 1e-6, what


# ========================================================================================================== forward
@pytest.mark.parametrize("F", SIZES_F)
def test_kernel_equals_the_definition_one_mesh(F):
    """Every S on one state tensor: the calls use successive draws, and leave the counter one higher each."""
    d = _d()
    vp, fp = blob(F, 0)
    state = _state(11, 5, d)
    for k, S in enumerate(SIZES_S):
        _check_forward("F %d S %d" % (F, S), _run(state, vp, fp, [0, F], S, d), 11, 5 + k, vp, fp, [0, F], S)
    assert state.tolist() == [11, 5 + len(SIZES_S)]


@pytest.mark.parametrize("S", SIZES_S)
def test_kernel_equals_the_definition_three_unequal_meshes(S):
    """A list of unequal meshes -- 257 faces with zero-area faces first, in the middle and last; no faces; 1025 faces
    with zero-area faces across a chunk edge -- with int64 and float faces, the table on the host and on the device, and
    a seed and a draw that use the high words of the key and the counter."""
    d = _d()
    vp, fp, first, _ = pack([blob(257, 1, zero_at=(0, 1, 128, -1)), (blob(8, 2)[0], blob(8, 2)[1][:0]),
                             blob(1025, 3, zero_at=(1023, 1024))])
    seed, draw = (0x1234ABCD << 32) | 77, (3 << 32) | 9
    for dtype, on_dev in ((torch.int64, False), (torch.float32, True)):
        state = _state(seed, draw, d)
        got = _run(state, vp, fp, first, S, d, faces_dtype=dtype, first_on_device=on_dev)
        _check_forward("N 3 S %d %s" % (S, dtype), got, seed, draw, vp, fp, first, S)
        assert (got[1][1] == -1).all() and not got[0][1].any() and not got[2][1].any()
        zero = [first[0], first[0] + 1, first[0] + 128, first[1] - 1, first[2] + 1023, first[2] + 1024]
        assert not np.isin(got[1], zero).any()
        assert state.tolist() == [seed, draw + 1]


def test_shim_on_the_gpu_and_default_sampler():
    """sample_points_from_meshes(sampler=) and default_sampler: the definition's points; normals of the drawn faces,
    zeros for the mesh without area; float faces as the reference stores them."""
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim import ops as shim_ops
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.structures import Meshes
    from acfm_video_3d_reconstruction_amd.surface_sampling import SurfaceSampler, surface_sample_host
    d = _d()
    parts = [blob(65, 4), (TWO_V, TWO_F[:0]), (TWO_V, TWO_F)]
    vp, fp, first, _ = pack(parts)
    ms = Meshes(verts=[torch.tensor(v, device=d) for v, _ in parts], faces=[torch.from_numpy(f).float().to(d) for _, f in parts])
    s = SurfaceSampler(seed=31)
    pts, nrm = shim_ops.sample_points_from_meshes(ms, 70, return_normals=True, sampler=s)
    with shim_ops.default_sampler(s):
        again = shim_ops.sample_points_from_meshes(ms, 70)
    assert s.state_on(d).tolist() == [31, 2]
    for t, got in ((0, pts), (1, again)):
        rp, rf, ruv = surface_sample_host(31, t, vp, fp, first, 70)
        assert float(np.abs(got.cpu().numpy() - rp).max()) <= 1e-6
    rp, rf, ruv = surface_sample_host(31, 0, vp, fp, first, 70)
    _, tri = weights64(vp, fp, np.where(rf >= 0, rf, 0), ruv)
    n = np.cross(tri[:, :, 1] - tri[:, :, 0], tri[:, :, 2] - tri[:, :, 0])
    n = n / np.linalg.norm(n, axis=-1, keepdims=True)
    n[rf < 0] = 0
    np.testing.assert_allclose(nrm.cpu().numpy(), n, atol=1e-5)
    assert torch.equal(nrm[2], torch.tensor([0, 0, 1.0], device=d).expand(70, 3))


# ========================================================================================================= backward
def _check_backward(what, gv, vp, fp, fidx, uv, g):
    ref = grad_reference(vp, fp, fidx, uv, g)
    live = fidx >= 0
    w, _ = weights64(vp, fp, np.where(live, fidx, 0), uv)
    mag, gmag, cnt = np.zeros_like(ref), np.zeros_like(ref), np.zeros(ref.shape[0])
    ids = fp[fidx[live]]
    g64 = g.astype(np.float64)[live][:, None, :]
    np.add.at(mag, ids.reshape(-1), np.abs(w[live][:, :, None] * g64).reshape(-1, 3))
    np.add.at(gmag, ids.reshape(-1), np.abs(np.ones((1, 3, 1)) * g64).reshape(-1, 3))
    np.add.at(cnt, ids.reshape(-1), 1.0)
    bound = (cnt[:, None] + 1.0) * 2.0 ** -24 * mag + 2.0 * 2.0 ** -24 * gmag
    err = np.abs(gv.astype(np.float64) - ref)
    worst = float((err / np.maximum(bound, 1e-300))[bound > 0].max()) if (bound > 0).any() else 0.0
    print("%s: max err %.2e, largest share of the summation bound %.3f, up to %d terms per vertex"
          % (what, float(err.max()), worst, int(cnt.max())))
    assert np.isfinite(gv).all(), what
    assert not gv[cnt == 0].any(), "%s: rows no sample touches must be exactly 0" % what
    assert (err <= bound).all(), what


BWD_CASES = {
    # name: (meshes, S, verts_per_mesh hint)
    "F1-S1000-lds": (lambda: [blob(1, 5)], 1000, 8),
    "F1-S1000-global": (lambda: [blob(1, 5)], 1000, 0),
    "two-equal-lds": (lambda: [blob(65, 6), blob(65, 7)], 257, 21),
    "three-unequal-global": (lambda: [blob(257, 1, zero_at=(0, 128, -1)), (blob(8, 2)[0], blob(8, 2)[1][:0]), blob(64, 8)], 65, 0),
    "hint-that-does-not-divide": (lambda: [blob(65, 6), blob(30, 8)], 64, 21),      # 21 + 10 vertices
    "V12800-lds": (lambda: [_wide(BWD_LDS_MAX_V)], 1000, BWD_LDS_MAX_V),
    "V12801-global": (lambda: [_wide(BWD_LDS_MAX_V + 1)], 1000, BWD_LDS_MAX_V + 1),
}


def _wide(V):
    """300 faces over V vertices, the last vertex among them: either side of the backward's LDS bound."""
    rng = np.random.default_rng(V)
    verts = rng.uniform(-1, 1, (V, 3)).astype(np.float32)
    faces = np.stack([rng.permutation(V)[:3] for _ in range(300)]).astype(np.int64)
    faces[7] = [V - 1, 0, V // 2]
    return verts, faces


@pytest.mark.parametrize("name", sorted(BWD_CASES))
def test_backward_against_float64(name):
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    make, S, vpm = BWD_CASES[name]
    vp, fp, first, vfirst = pack(make())
    N = len(first) - 1
    rng = np.random.default_rng(len(name))
    g = rng.uniform(-1, 1, (N, S, 3)).astype(np.float32)
    tv = torch.tensor(vp, device=d, requires_grad=True)
    pts, fidx, uv = ops.sample_surface_uv(_state(3, 1, d), tv, torch.from_numpy(fp).to(d), torch.tensor(first), S, vpm)
    gv, = torch.autograd.grad(pts, tv, torch.tensor(g, device=d))
    assert gv.shape == tv.shape
    _check_forward(name, (pts.detach().cpu().numpy(), fidx.cpu().numpy(), uv.cpu().numpy()), 3, 1, vp, fp, first, S)
    _check_backward(name, gv.cpu().numpy(), vp, fp, fidx.cpu().numpy(), uv.cpu().numpy(), g)


# ================================================================================================== capture, guards
def test_one_captured_call_replays_the_next_draws():
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    vp, fp, first, _ = pack([blob(257, 1, zero_at=(0, 128, -1)), blob(65, 4)])
    S = 300
    tv, tf, t1 = torch.tensor(vp, device=d, requires_grad=True), torch.from_numpy(fp).to(d), torch.tensor(first)
    state = _state(8, 0, d)
    g = torch.ones((2, S, 3), device=d)

    def once():
        pts, fidx, uv = ops.sample_surface_uv(state, tv, tf, t1, S)
        gv, = torch.autograd.grad(pts, tv, g)
        return pts, fidx, uv, gv

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        once()                                               # the table and the allocator exist before the capture
    torch.cuda.current_stream().wait_stream(side)
    assert state.tolist() == [8, 1]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pts, fidx, uv, gv = once()
    seen = []
    for t in (1, 2, 3):
        graph.replay()
        got = (pts.detach().cpu().numpy(), fidx.cpu().numpy(), uv.cpu().numpy())
        _check_forward("replay at draw %d" % t, got, 8, t, vp, fp, first, S)
        _check_backward("replay at draw %d" % t, gv.cpu().numpy(), vp, fp, got[1], got[2], np.ones((2, S, 3), np.float32))
        assert state.tolist() == [8, t + 1]
        seen.append(got[1])
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])


@pytest.mark.parametrize("name", ["two-equal-lds", "three-unequal-global"])
def test_guards(name):
    """Forward and backward on hostile, fenced memory (tests/guards.py run_case): fences intact, nothing the op
    allocates left unwritten, points / face ids / (u, v) bit-identical between the runs; the gradient (float atomics)
    is held to its float64 reference in every run."""
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    make, S, vpm = BWD_CASES[name]
    vp, fp, first, _ = pack(make())
    N = len(first) - 1
    tf, t1 = torch.from_numpy(fp).to(d), torch.tensor(first)
    g = np.random.default_rng(5).uniform(-1, 1, (N, S, 3)).astype(np.float32)

    def fn(inp):
        tv = inp(torch.tensor(vp, device=d, requires_grad=True))
        state = _state(2, 6, d)
        pts, fidx, uv = ops.sample_surface_uv(state, tv, tf, t1, S, vpm)
        gv, = torch.autograd.grad(pts, tv, inp(torch.tensor(g, device=d)))
        _check_backward(name, gv.cpu().numpy(), vp, fp, fidx.cpu().numpy(), uv.cpu().numpy(), g)
        return dict(pts=pts, fidx=fidx, uv=uv, gv=gv, state=state)
    plain, _ = guards.run_case(fn, loose=("gv",))
    _check_forward(name, (plain["pts"].detach().cpu().numpy(), plain["fidx"].cpu().numpy(), plain["uv"].cpu().numpy()),
                   2, 6, vp, fp, first, S)
    assert plain["state"].tolist() == [2, 7]


# ============================================================================================================ the fit
@pytest.mark.parametrize("use_graph", [False, True])
def test_fit_sphere_to_ellipsoid(use_graph):
    """30 iterations on ico_sphere(2) with 500 samples a side, eager and with one captured iteration replayed: finite,
    the chamfer term falls, and the draw counter ends at exactly 2 x 30.  (The two runs differ in the order of float
    atomic additions only; they are not compared bit for bit.)"""
    from acfm_video_3d_reconstruction_amd import template_fit
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.utils import ico_sphere
    from acfm_video_3d_reconstruction_amd.surface_sampling import SurfaceSampler
    d = _d()
    m = ico_sphere(2)
    v, f = m.verts_list()[0].numpy(), m.faces_list()[0].numpy()
    target = v * np.array([1.0, 0.6, 0.4], np.float32) * 2.0 + np.array([0.5, -1.0, 0.25], np.float32)
    s = SurfaceSampler(seed=13)
    out, hist = template_fit.fit_verts_to_mesh(v, f, target, f, n_iter=30, num_samples=500, sampler=s, use_graph=use_graph,
                                               device=d, return_history=True)
    print("use_graph=%s: chamfer, edge, normal, laplacian at steps 0 / 29: %s / %s" % (use_graph, hist[0], hist[-1]))
    assert out.shape == v.shape and np.isfinite(out).all() and np.isfinite(hist).all() and hist.shape == (30, 4)
    assert hist[-1, 0] < hist[0, 0]
    assert s.state_on(d).tolist() == [13, 2 * 30]
