"""pytorch3d_shim.ops.knn_points / knn_gather and chamfer_distance with normals on host tensors (no GPU), against the
float64 restatements of tests/knn_cases.py (see its docstring for the bars and the tie bookkeeping).  Every input of
tests/test_gpu_knn.py is first put through the float32 host path here, at the GPU tests' bars."""
import ctypes
import sys

import numpy as np
import pytest
import torch

import knn_cases as kc


def test_inputs_have_few_hesitant_rows():
    """The cap on what the comparisons leave out: at most 2 % of a case's query rows hesitate, for every input."""
    for name in kc.ALL_NAMES:
        r = kc.reference(name)
        rows, hes = r["hesitant"].size, int(r["hesitant"].sum())
        if hes:
            print("%s: %d hesitant rows of %d" % (name, hes, rows))
        assert hes <= kc.TIE_SHARE * rows, name


@pytest.mark.parametrize("name", kc.ALL_NAMES)
def test_host_path(name):
    dists, idx, g1, g2 = kc.host(name)
    kc.check_forward(name + " host", dists, idx, name)
    kc.check_backward(name + " host", g1, g2, name)


def test_reference_and_host_order_copies_by_index():
    """The float64 helper itself lists bit-identical copies in index order, before a farther point; the query that
    equals them is at distance exactly 0 from each; two equal queries get equal rows."""
    r = kc.reference("ties-k8")
    assert r["idx"][0, 5, :5].tolist() == kc.TIE_COPIES and not r["dists"][0, 5, :5].any() and r["dists"][0, 5, 5] > 0
    assert not r["hesitant"][0, 5]
    dists, idx, _, _ = kc.host("ties-k8")
    assert idx[0, 5, :5].tolist() == kc.TIE_COPIES and not dists[0, 5, :5].any()
    assert np.array_equal(idx[0, 6], idx[0, 9]) and np.array_equal(dists[0, 6], dists[0, 9])
    for K in (1, 2, 4):                                                       # more copies than K
        assert kc.host("ties-k%d" % K)[1][0, 5].tolist() == kc.TIE_COPIES[:K]


def test_lengths_padding_on_the_host():
    """NaN beyond the lengths never reaches a result; columns past lengths2 and rows past lengths1 are 0 / 0."""
    c = kc.cloud_case("lengths")
    dists, idx, g1, g2 = kc.host("lengths-k8")
    assert np.isfinite(dists).all() and np.isfinite(g1).all() and np.isfinite(g2).all()
    assert not dists[0, :, 5:].any() and dists[0, :70, :5].all()              # lengths2[0] = 5 < K
    assert not dists[3].any() and not dists[4].any() and not idx[3].any()     # lengths2[3] = 0, lengths1[4] = 0
    assert not dists[1, 1:].any() and c.l1[1] == 1 and c.l2[2] == 1


@pytest.mark.parametrize("D", [1, 2, 5])
def test_host_path_any_dimension(D):
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.ops import knn_points
    rng = np.random.default_rng(40 + D)
    p1, p2 = rng.uniform(-1, 1, (2, 9, D)).astype(np.float32), rng.uniform(-1, 1, (2, 21, D)).astype(np.float32)
    out = knn_points(torch.tensor(p1), torch.tensor(p2), K=4)
    d = ((p1.astype(np.float64)[:, :, None, :] - p2.astype(np.float64)[:, None, :, :]) ** 2).sum(-1)
    order = np.argsort(d, axis=2, kind="stable")[:, :, :4]
    assert np.array_equal(out.idx.numpy(), order) and out.knn is None
    np.testing.assert_allclose(out.dists.numpy(), np.take_along_axis(d, order, 2), rtol=kc.DIST_RTOL, atol=0)


def test_shim_arguments_and_install():
    from acfm_video_3d_reconstruction_amd import pytorch3d_shim
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.ops import knn_gather, knn_points
    c = kc.cloud_case("lengths")
    p1, p2 = torch.tensor(c.p1), torch.tensor(c.p2)
    l1, l2 = torch.tensor(c.l1), torch.tensor(c.l2)
    a = knn_points(p1, p2, l1, l2, K=8, return_nn=True)
    b = knn_points(p1, p2, l1, l2, 8, version=2, return_sorted=False)
    assert type(a).__name__ == "KNN" and a._fields == ("dists", "idx", "knn") and b.knn is None
    assert torch.equal(a.dists, b.dists) and torch.equal(a.idx, b.idx)
    assert a.knn.shape == (6, 70, 8, 3) and torch.equal(a.knn, knn_gather(p2, a.idx, l2)) and bool(torch.isfinite(a.knn).all())
    assert not a.knn[0, :, 5:].any()                                          # k >= lengths2[0]
    saved = {k: sys.modules[k] for k in list(sys.modules) if k == "pytorch3d" or k.startswith("pytorch3d.")}
    try:
        pytorch3d_shim.install(force=True)
        from pytorch3d.ops import knn_gather as g2, knn_points as k2
        assert k2 is knn_points and g2 is knn_gather
    finally:
        for k in [k for k in sys.modules if k == "pytorch3d" or k.startswith("pytorch3d.")]:
            del sys.modules[k]
        sys.modules.update(saved)


@pytest.mark.parametrize("U", [1, 3, 7])
def test_knn_gather_on_the_host(U):
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.ops import knn_gather
    rng = np.random.default_rng(50 + U)
    x = rng.uniform(-1, 1, (3, 11, U)).astype(np.float32)
    idx = rng.integers(0, 11, (3, 6, 4))
    lengths = np.array([11, 2, 0])
    want, ok = kc.gather_reference(x, idx, lengths)
    X = torch.tensor(x, requires_grad=True)
    for i in (torch.from_numpy(idx), torch.from_numpy(idx).int()):
        out = knn_gather(X, i, torch.from_numpy(lengths))
        assert np.array_equal(out.detach().numpy().astype(np.float64), want)
    go = rng.uniform(-1, 1, out.shape).astype(np.float32)
    out.backward(torch.tensor(go))
    np.testing.assert_allclose(X.grad.numpy(), kc.gather_grad_reference(go, idx, ok, 11), rtol=1e-6, atol=1e-6)
    assert np.array_equal(knn_gather(X, torch.from_numpy(idx)).detach().numpy().astype(np.float64),
                          kc.gather_reference(x, idx, None)[0])
    bad = torch.from_numpy(idx).clone()
    bad[0, 0, 0] = 11
    with pytest.raises((RuntimeError, IndexError)):                           # as torch.gather does
        knn_gather(X, bad)


def test_refusals():
    from acfm_video_3d_reconstruction_amd import ops
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.ops import knn_gather, knn_points
    p1, p2 = torch.zeros(2, 4, 3), torch.zeros(2, 5, 3)
    with pytest.raises(ValueError, match="same batch dimension"):
        knn_points(p1, torch.zeros(3, 5, 3))
    with pytest.raises(ValueError, match="same point dimension"):
        knn_points(p1, torch.zeros(2, 5, 2))
    with pytest.raises(ValueError, match="lengths1"):
        knn_points(p1, p2, lengths1=torch.tensor([1, 2, 3]))
    with pytest.raises(ValueError, match="lengths2"):
        knn_points(p1, p2, lengths2=torch.tensor([1]))
    with pytest.raises(ValueError, match="K must be"):
        knn_points(p1, p2, K=0)
    with pytest.raises(ValueError, match="at least one"):
        knn_points(torch.zeros(2, 0, 3), p2)
    with pytest.raises(ValueError, match="idx"):
        knn_gather(p1, torch.zeros(3, 2, 2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):                # the kernels' operators take GPU tensors only
        ops.knn_points(p1, p2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.knn_gather(p1, torch.zeros(2, 2, 2, dtype=torch.int64))


def test_entry_points_refuse_bad_sizes_before_any_launch():
    """ACFM_E_BADARG (1) for K outside 1..32, non-positive sizes and element counts past the index arithmetic; nothing
    is launched or read (the pointers are never dereferenced)."""
    from acfm_video_3d_reconstruction_amd import _lib
    _lib.build()
    h, p = _lib.lib(), ctypes.c_void_p(0x1000)
    big = 2 ** 31 - 1
    for N, P1, P2, K in ((1, 4, 4, 0), (1, 4, 4, 33), (0, 4, 4, 1), (1, 0, 4, 1), (1, 4, -1, 1), (65536, 4, 4, 1)):
        assert h.acfm_knn_points(p, p, None, None, N, P1, P2, K, p, p, None) == 1, (N, P1, P2, K)
        assert h.acfm_knn_points_backward(p, p, None, None, p, p, N, P1, P2, K, p, p, None) == 1, (N, P1, P2, K)
    for N, M, U, L, K in ((0, 4, 3, 4, 1), (1, 0, 3, 4, 1), (1, 4, 0, 4, 1), (1, 4, 3, 0, 1), (1, 4, 3, 4, 0),
                          (big, 4, big, big, big), (2, 4, 1024, big, 1024), (big, big, big, 1, 1)):
        assert h.acfm_knn_gather(p, p, 1, None, N, M, U, L, K, p, None) == 1, (N, M, U, L, K)
        assert h.acfm_knn_gather_backward(p, p, 0, None, N, M, U, L, K, p, None) == 1, (N, M, U, L, K)


# ===================================================================================== chamfer_distance with normals
@pytest.mark.parametrize("pr,br,weighted", kc.REDUCTIONS)
@pytest.mark.parametrize("name", kc.NORMAL_CASES)
def test_chamfer_normals_host_path(name, pr, br, weighted):
    kc.check_normals("%s %s/%s host" % (name, pr, br), kc.normals_host(name, pr, br, weighted), name, pr, br, weighted)


def test_chamfer_normals_zero_normal_and_empty_cloud():
    """The zero normals (cosine_similarity's eps branch) give a term of exactly 1 and a zero gradient; a point whose
    other cloud is empty gathers a zero normal: term 1 as well, finite everywhere."""
    from test_shim_template_fit import chamfer_case
    c = chamfer_case("lengths")
    loss, plain, ln, gxn, gyn, _ = kc.normals_host("lengths", "sum", None, False)
    assert np.isfinite(ln).all() and not gxn[0, 2].any() and not gyn[0, 1].any()
    assert ln[3] == c.xl[3] and ln[4] == c.yl[4]                              # y_lengths[3] = 0, x_lengths[4] = 0
    assert not gxn[3].any() and not gyn[4].any()


def test_chamfer_one_normal_alone_is_refused():
    """tests/test_shim_template_fit.py::test_refusals pins this: one of the two normals alone is a ValueError that
    names it."""
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.loss import chamfer_distance
    x, y = torch.zeros(2, 4, 3), torch.zeros(2, 5, 3)
    with pytest.raises(ValueError, match="together"):
        chamfer_distance(x, y, x_normals=torch.zeros(2, 4, 3))
    with pytest.raises(ValueError, match="shapes of x / y"):
        chamfer_distance(x, y, x_normals=torch.zeros(2, 4, 3), y_normals=torch.zeros(2, 4, 3))
