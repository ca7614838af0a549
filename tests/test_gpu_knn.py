"""The kernels of csrc/acfm_knn.hip on the GPU -- k_knn<1..32>, k_knn_bwd and its global-atomic form k_knn_bwd_global,
k_knn_gather / k_knn_gather_bwd -- through the shim's public functions, and chamfer_distance with normals, against the
float64 helpers of tests/knn_cases.py, whose CPU tests (tests/test_knn.py) put every input used here through the
float32 host path first.  Bars and tie bookkeeping: see knn_cases.py; every measured figure is printed before it is
asserted.

The sizes at which the kernels change path, each with a case either side (the queries at 64 points):"""
import numpy as np
import pytest
import torch

import guards
import knn_cases as kc

KNN_Q = kc.KNN_Q                            # 64 query points per workgroup: 63 / 64 / 65 queries
KNN_ROUND = kc.KNN_ROUND                    # 1024 candidates per round (four waves x a 256-point tile): 1024 / 1025
CH_BWD_LDS_MAX_P = kc.CH_BWD_LDS_MAX_P      # grad_p2 in LDS up to 12800 points of p2 (150 KB); 12801: global atomics
KNN_BWD_LDS_MAX_SLOTS = kc.KNN_BWD_LDS_MAX_SLOTS   # ... and up to 16384 slots P1 K: 512 x 32 in LDS, 513 x 32 global

pytestmark = pytest.mark.gpu


def _d():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _knn(name):
    dists, idx, g1, g2 = kc.run_knn(name, _d())
    kc.check_forward(name, dists, idx, name)
    kc.check_backward(name, g1, g2, name, host_grads=kc.host(name)[2:])
    return dists, idx, g1, g2


@pytest.mark.parametrize("name", kc.SIZE_NAMES)
def test_knn_sizes_and_every_k(name):
    """(P1, P2) either side of the 64-query workgroup and of one tile, N = 1 and 3, every instantiation of K and
    K = 3, 5, 20, 31 in between; where P2 < K the columns past P2 are padding."""
    _knn(name)


@pytest.mark.parametrize("name", kc.BOUND_NAMES)
def test_knn_round_and_lds_bounds(name):
    """Either side of the 1024-candidate round of the forward and of the backward's two LDS bounds (module docstring)."""
    assert KNN_ROUND == 1024 and 12 * CH_BWD_LDS_MAX_P == 150 * 1024 and KNN_Q == 64 and KNN_BWD_LDS_MAX_SLOTS == 512 * 32
    _knn(name)


@pytest.mark.parametrize("name", kc.SMALL_P2_NAMES)
def test_knn_fewer_candidates_than_k(name):
    """P2 < K, P2 == K and P2 == K + 1."""
    dists, idx, _, _ = _knn(name)
    c, K = kc.cloud_case(kc.split(name)[0]), kc.split(name)[1]
    if c.P2 < K:
        assert not dists[:, :, c.P2:].any() and not idx[:, :, c.P2:].any() and dists[:, :, :c.P2].all()


@pytest.mark.parametrize("name", kc.LENGTH_NAMES)
def test_knn_lengths_and_nan_padding(name):
    """NaN beyond every length on both sides, lengths of 1 and of 0 on either side, lengths2 < K for some clouds only:
    everything finite, padded slots and padded gradient rows exactly 0 (check_forward / check_backward assert it)."""
    dists, idx, g1, g2 = _knn(name)
    assert np.isfinite(g1).all() and np.isfinite(g2).all()
    assert not dists[3].any() and not dists[4].any() and not g1[3].any() and not g2[4].any()


@pytest.mark.parametrize("name", kc.TIE_NAMES)
def test_knn_ties_and_duplicates(name):
    """Five bit-identical copies of a p2 point spread over the four waves' quarters, more of them than K; a query equal
    to them; two equal queries.  The copies come out in index order at distance exactly 0."""
    dists, idx, _, _ = _knn(name)
    K = kc.split(name)[1]
    m = min(K, len(kc.TIE_COPIES))
    assert idx[0, 5, :m].tolist() == kc.TIE_COPIES[:m] and not dists[0, 5, :m].any()
    assert np.array_equal(idx[0, 6], idx[0, 9]) and np.array_equal(dists[0, 6], dists[0, 9])
    assert np.array_equal(idx, kc.reference(name)["idx"])


def test_knn_k1_agrees_with_chamfer_nearest():
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    for name in ("n3-257x1000-k1", "lengths-k1"):
        c, r = kc.cloud_case(kc.split(name)[0]), kc.reference(name)
        p1, p2 = torch.tensor(c.p1, device=d), torch.tensor(c.p2, device=d)
        l1 = None if c.l1 is None else torch.tensor(c.l1, device=d)
        l2 = None if c.l2 is None else torch.tensor(c.l2, device=d)
        dists, idx = ops.knn_points(p1, p2, l1, l2, K=1)
        sums, ix, _ = ops.chamfer_nearest(p1, p2, l1, l2)
        live = torch.from_numpy(r["valid"][..., 0] & ~r["hesitant"]).to(d)
        assert bool((idx[..., 0][live] == ix.long()[live]).all()), name
        got, want = dists.double().sum((1, 2)).cpu().numpy(), sums[:, 0].double().cpu().numpy()
        print("%s: per-cloud sums %s vs chamfer %s" % (name, got, want))
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=0)


def test_knn_forward_is_reproducible_and_refusals_by_name():
    from acfm_video_3d_reconstruction_amd import ops
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.ops import knn_points
    d = _d()
    c = kc.cloud_case("n3-257x1000")
    p1, p2 = torch.tensor(c.p1, device=d), torch.tensor(c.p2, device=d)
    a, b = ops.knn_points(p1, p2, K=20), ops.knn_points(p1, p2, K=20)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for fn in (ops.knn_points, knn_points):
        with pytest.raises(ValueError, match="D = 3"):
            fn(p1[..., :2], p2[..., :2])
        with pytest.raises(ValueError, match="float32"):
            fn(p1.double(), p2.double())
        for K in (0, 33):
            with pytest.raises(ValueError, match="K must be in 1..32"):
                fn(p1, p2, K=K)
        with pytest.raises(ValueError, match="at least one"):
            fn(p1[:, :0], p2)
        with pytest.raises(ValueError, match="lengths2"):
            fn(p1, p2, lengths2=torch.tensor([1, 2], device=d))


def test_shim_on_the_gpu():
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.ops import knn_gather, knn_points
    d = _d()
    c = kc.cloud_case("lengths")
    p1, p2 = torch.tensor(c.p1, device=d), torch.tensor(c.p2, device=d)
    l1, l2 = torch.tensor(c.l1, device=d), torch.tensor(c.l2, device=d)
    a = knn_points(p1, p2, l1, l2, K=8, return_nn=True)
    b = knn_points(p1, p2, l1, l2, 8, version=3, return_sorted=False)
    assert torch.equal(a.dists, b.dists) and torch.equal(a.idx, b.idx) and b.knn is None
    assert a.knn.shape == (6, 70, 8, 3) and torch.equal(a.knn, knn_gather(p2, a.idx, l2))
    assert bool(torch.isfinite(a.knn).all()) and not a.knn[0, :, 5:].any()
    host = kc.host("lengths-k8")
    assert np.array_equal(a.idx.cpu().numpy(), host[1])


# ======================================================================================================== knn_gather
@pytest.mark.parametrize("U", [1, 3, 4, 7, 64])
@pytest.mark.parametrize("idx_dtype", [torch.int32, torch.int64])
def test_knn_gather(U, idx_dtype):
    """Values are copies (bit-exact); lengths smaller than K zero the columns past them; a planted index of -1, of M and
    of the guards' poison pattern yields zeros and sends no gradient (the kernel tests the index before it uses it);
    the gradient against index_add in float64."""
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    N, M, L, K = 3, 37, 70, 5
    rng = np.random.default_rng(60 + U)
    x = rng.uniform(-1, 1, (N, M, U)).astype(np.float32)
    idx = rng.integers(0, M, (N, L, K))
    idx[0, 0, 0], idx[1, 3, 2], idx[2, 69, 4] = -1, M, guards.pattern_word("A", idx_dtype)[1]
    idx[0, 1, 1] = guards.pattern_word("B", idx_dtype)[1]
    lengths = np.array([M, 3, 0])
    X = torch.tensor(x, device=d, requires_grad=True)
    I = torch.tensor(idx, device=d).to(idx_dtype)
    go = rng.uniform(-1, 1, (N, L, K, U)).astype(np.float32)
    for ln in (lengths, None):
        want, ok = kc.gather_reference(x, idx, ln)
        assert not ok[0, 0, 0] and not ok[1, 3, 2] and not ok[2, 69, 4] and not ok[0, 1, 1]
        out = ops.knn_gather(X, I, None if ln is None else torch.tensor(ln, device=d))
        assert out.shape == (N, L, K, U) and np.array_equal(out.detach().cpu().numpy().astype(np.float64), want)
        (gx,) = torch.autograd.grad(out, X, torch.tensor(go, device=d))
        ref = kc.gather_grad_reference(go, idx, ok, M)
        err = float(np.abs(gx.cpu().numpy() - ref).max())
        print("U %d %s lengths %s: grad max abs err %.2e" % (U, idx_dtype, ln is not None, err))
        # each entry is a float32 sum of about L K / M = 10 terms in [-1, 1]: 1e-5 of the largest entry is 30 eps
        np.testing.assert_allclose(gx.cpu().numpy(), ref, rtol=1e-6, atol=1e-5 * float(np.abs(ref).max()))
    with pytest.raises(ValueError, match="float32"):
        ops.knn_gather(X.double(), I)
    with pytest.raises(ValueError, match="int64 or int32"):
        ops.knn_gather(X, I.short())


def test_knn_gather_takes_chamfer_indices_with_unwritten_rows():
    """ops.chamfer_nearest leaves index rows past a length unwritten by contract: under poison they reach knn_gather,
    which must answer zeros there."""
    from acfm_video_3d_reconstruction_amd import ops
    from test_shim_template_fit import chamfer_case
    d = _d()
    c = chamfer_case("lengths")
    x, y = torch.tensor(c.x, device=d), torch.tensor(c.y, device=d)
    xl, yl = torch.tensor(c.xl, device=d), torch.tensor(c.yl, device=d)
    feats = torch.tensor(np.random.default_rng(3).uniform(1, 2, (c.N, c.P2, 3)).astype(np.float32), device=d)
    with guards.armed("A") as g:
        _, ix, _ = ops.chamfer_nearest(x, y, xl, yl)
        out = ops.knn_gather(feats, ix[:, :, None], yl)
    g.check()
    pad = torch.from_numpy(np.arange(c.P1)[None] >= np.asarray(c.lx)[:, None]).to(d)
    assert bool(torch.isfinite(out).all()) and not out[:, :, 0][pad].any()
    assert bool((out[0, :70, 0] >= 1).all())


# ===================================================================================== chamfer_distance with normals
@pytest.mark.parametrize("pr,br,weighted", kc.REDUCTIONS)
@pytest.mark.parametrize("name", kc.NORMAL_CASES)
def test_chamfer_with_normals(name, pr, br, weighted):
    """The GPU path against float64 and against the host path on the chamfer suite's "lengths" and "ties" inputs and one
    plain size, unit and non-unit normals and a zero normal on each side; both reductions, with and without weights.
    `loss` keeps the bits it has without normals; the points get no gradient from the normal term."""
    got = kc.run_normals(name, _d(), pr, br, weighted)
    host = kc.normals_host(name, pr, br, weighted)
    kc.check_normals("%s %s/%s" % (name, pr, br), got, name, pr, br, weighted, host_run=host)
    # two float32 sums of at most 130 terms, each term within 8 eps: the two paths are within 1e-5 of each other
    np.testing.assert_allclose(got[2], host[2], rtol=1e-5, atol=0)


def test_chamfer_one_normal_alone_on_the_gpu():
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.loss import chamfer_distance
    d = _d()
    x, y = torch.rand(2, 4, 3, device=d), torch.rand(2, 5, 3, device=d)
    with pytest.raises(ValueError, match="together"):
        chamfer_distance(x, y, y_normals=torch.rand(2, 5, 3, device=d))


# ================================================================================================ memory and capture
def test_knn_memory_stays_linear():
    """N = 1, P1 = P2 = 20000, K = 8: the peak of forward + backward stays below outputs + gradients + 1 MB above what
    the inputs hold (the [P1,P2] distance matrix alone would be 1.6 GB)."""
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    P, K = 20000, 8
    gen = torch.Generator(device="cpu").manual_seed(9)
    p1 = torch.rand(1, P, 3, generator=gen).to(d).requires_grad_(True)
    p2 = torch.rand(1, P, 3, generator=gen).to(d).requires_grad_(True)
    g = torch.rand(1, P, K, generator=gen).to(d)
    ops.knn_points(p1[:, :64].detach(), p2[:, :64].detach(), K=K)             # code objects loaded before measuring
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(d)
    before = torch.cuda.memory_allocated(d)
    dists, idx = ops.knn_points(p1, p2, K=K)
    dists.backward(g)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(d) - before
    budget = dists.numel() * 4 + idx.numel() * 8 + 2 * p1.numel() * 4 + (1 << 20)
    print("peak above the inputs %.2f MB, budget %.2f MB" % (peak / 2 ** 20, budget / 2 ** 20))
    assert peak <= budget
    assert bool(torch.isfinite(p1.grad).all()) and bool(torch.isfinite(p2.grad).all())
    assert bool((idx >= 0).all()) and bool((idx < P).all()) and bool((dists[..., 1:] >= dists[..., :-1]).all())


def test_knn_captured_in_a_graph():
    """One eager call, then the same call -- knn_points with return_nn, and the backward of both results -- captured on
    one stream and replayed twice on changed inputs: the eager results (the float-atomic gradient of p2 to 1e-6 of its
    largest entry, everything else bit for bit)."""
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.ops import knn_points
    d = _d()
    c = kc.cloud_case("n3-257x1000")
    rng = np.random.default_rng(12)
    p1 = torch.tensor(c.p1, device=d, requires_grad=True)
    p2 = torch.tensor(c.p2, device=d, requires_grad=True)
    l2 = torch.tensor([1000, 7, 600], device=d)
    gd = torch.tensor(rng.uniform(-1, 1, (3, 257, 8)).astype(np.float32), device=d)
    gk = torch.tensor(rng.uniform(-1, 1, (3, 257, 8, 3)).astype(np.float32), device=d)

    def step():
        out = knn_points(p1, p2, None, l2, K=8, return_nn=True)
        g1, g2 = torch.autograd.grad([out.dists, out.knn], [p1, p2], [gd, gk])
        return out.dists, out.idx, out.knn, g1, g2

    step()                                                                    # eager first: code objects loaded
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for r in range(2):
        with torch.no_grad():
            p1.copy_(torch.flip(p1, (0, 1)) * (1.0 + 0.25 * r))
            p2.copy_(torch.flip(p2, (1,)) - 0.125)
            l2.copy_(torch.flip(l2, (0,)))
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in captured]
        eager = step()
        for i, (a, e) in enumerate(zip(got, eager)):
            if i == 4:
                assert float((a - e).abs().max()) <= 1e-6 * float(e.abs().max())
            else:
                assert torch.equal(a, e), i
