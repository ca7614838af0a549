"""Inputs, float64 brute-force references and tie bookkeeping of the K-nearest-neighbour tests (a helper of
tests/test_knn.py, tests/test_gpu_knn.py and tests/test_gpu_guards_knn.py; not a conftest).

The reference restates the documented behaviour of PyTorch3D 0.3.0's pytorch3d.ops.knn_points / knn_gather: for every
point of p1[n, :lengths1[n]] the min(K, lengths2[n]) nearest points of p2[n, :lengths2[n]] by squared distance,
ascending; every other slot of dists / idx is 0.  PyTorch3D is not installed where this suite runs, so the restatement
could NOT be run against the package itself.  PyTorch3D leaves the order among equal distances open; this package
documents the lower index first, and the reference (numpy's stable argsort in float64) holds it to that.

Bars (those of tests/test_shim_template_fit.py, whose helpers are imported): gradients rtol 1e-3 with atol = 1e-5 of
the largest reference entry, relative L2 <= max(1e-5, 4 x the host path's).  dists: rtol 1e-6 -- a float32
(dx dx + dy dy) + dz dz carries one rounding per difference (2^-24 relative each, doubled by the square), one per
product and one per sum: below 4 x 2^-23 = 4.8e-7 relative.

A row HESITATES if, in float64, two consecutive entries among its first min(K + 1, l2) sorted distances differ by at
most TIE_GAP = 1e-5 relative and the two points are not bit-identical copies (copies get the same distance in every
arithmetic, and must come out in index order).  Hesitant rows, and the p2 rows they hesitate between, are left out of
the index and gradient comparisons; they may not exceed TIE_SHARE = 2 % of a case's query rows, which
test_knn.py::test_inputs_have_few_hesitant_rows asserts for every input.  (A row has K chances to hesitate: the chamfer
suite's 0.5 % does not fit K = 32.)"""
import functools

import numpy as np
import torch

from test_shim_template_fit import TIE_GAP

DIST_RTOL = 1e-6
TIE_SHARE = 0.02
KNN_MAX_K = 32
K_INSTANCES = [1, 2, 4, 8, 16, 32]         # the instantiations of k_knn (csrc/acfm_knn.hip)
K_BETWEEN = [3, 5, 20, 31]                 # run the next instantiation and store its first K columns
K_ALL = sorted(K_INSTANCES + K_BETWEEN)
# the sizes at which the kernels take another path
KNN_Q = 64                                 # query points per workgroup
KNN_ROUND = 4 * 256                        # candidates per round: four waves x a tile of 256 (a second round past 1024)
CH_BWD_LDS_MAX_P = 12800                   # grad_p2 in LDS up to here (12 B per point); past it global atomics
KNN_BWD_LDS_MAX_SLOTS = 16384              # ... and while P1 K stays within this: 512 x 32 is the last LDS case

SIZE_PAIRS = [(1, 1), (1, 64), (63, 65), (64, 64), (65, 31), (257, 1000), (300, 2049)]
BOUND_PAIRS = [(64, KNN_ROUND), (64, KNN_ROUND + 1), (64, CH_BWD_LDS_MAX_P), (64, CH_BWD_LDS_MAX_P + 1)]
BOUND_KS = [3, 32]
SMALL_P2_RUNS = [(40, K - 1, K) for K in (2, 8, 31)] + [(40, K, K) for K in (1, 4, 16, 32)] + \
                [(40, K + 1, K) for K in (1, 5, 20, 32)]          # P2 < K, P2 == K, P2 == K + 1
LENGTH_KS = [1, 8, 32]
TIE_KS = [1, 2, 4, 8]
TIE_COPIES = [3, 7, 80, 160, 290]          # bit-identical points of p2[0]: the quarters of 300 are 75 points each

SIZE_NAMES = ["n%d-%dx%d-k%d" % (n, a, b, k) for n in (1, 3) for a, b in SIZE_PAIRS for k in K_ALL]
BOUND_NAMES = ["n1-%dx%d-k%d" % (a, b, k) for a, b in BOUND_PAIRS for k in BOUND_KS] + \
              ["n1-%dx64-k32" % (KNN_BWD_LDS_MAX_SLOTS // 32), "n1-%dx64-k32" % (KNN_BWD_LDS_MAX_SLOTS // 32 + 1)]
SMALL_P2_NAMES = ["n2-%dx%d-k%d" % r for r in SMALL_P2_RUNS]
LENGTH_NAMES = ["lengths-k%d" % k for k in LENGTH_KS]
TIE_NAMES = ["ties-k%d" % k for k in TIE_KS]
ALL_NAMES = SIZE_NAMES + BOUND_NAMES + SMALL_P2_NAMES + LENGTH_NAMES + TIE_NAMES


class KnnCase:
    def __init__(self, p1, p2, l1=None, l2=None):
        self.p1, self.p2, self.l1, self.l2 = p1, p2, l1, l2
        self.N, self.P1, self.P2 = p1.shape[0], p1.shape[1], p2.shape[1]
        self.lx = np.full(self.N, self.P1) if l1 is None else np.clip(l1, 0, self.P1)
        self.ly = np.full(self.N, self.P2) if l2 is None else np.clip(l2, 0, self.P2)


def split(name):
    """'n3-63x65-k5' -> ('n3-63x65', 5)"""
    base, k = name.rsplit("-k", 1)
    return base, int(k)


@functools.lru_cache(maxsize=None)
def cloud_case(base):
    if base == "lengths":     # NaN beyond every length; lengths of 1 and 0 on either side; l2 < K for some clouds only
        rng = np.random.default_rng(31)
        p1 = rng.uniform(-1, 1, (6, 70, 3)).astype(np.float32)
        p2 = rng.uniform(-1, 1, (6, 130, 3)).astype(np.float32)
        l1, l2 = np.array([70, 1, 33, 20, 0, 50]), np.array([5, 130, 1, 0, 9, 40])
        for n in range(6):
            p1[n, l1[n]:] = np.nan
            p2[n, l2[n]:] = np.nan
        return KnnCase(p1, p2, l1, l2)
    if base == "ties":        # five copies of p2[0,3], one per wave's quarter and two in the first; p1[0,5] equals them;
        rng = np.random.default_rng(32)                                       # p1[0,9] == p1[0,6]
        p1 = rng.uniform(-1, 1, (1, 40, 3)).astype(np.float32)
        p2 = rng.uniform(-1, 1, (1, 300, 3)).astype(np.float32)
        for j in TIE_COPIES[1:]:
            p2[0, j] = p2[0, 3]
        p1[0, 5] = p2[0, 3]
        p1[0, 9] = p1[0, 6]
        return KnnCase(p1, p2)
    n, rest = base.split("-")
    N, (P1, P2) = int(n[1:]), (int(v) for v in rest.split("x"))
    rng = np.random.default_rng(5000 * N + 11 * P1 + P2)
    return KnnCase(rng.uniform(-1, 1, (N, P1, 3)).astype(np.float32), rng.uniform(-1, 1, (N, P2, 3)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _sorted64(base):
    """Per cloud: (order [l1, m], distances [l1, m]) of the m = min(KNN_MAX_K + 1, l2) nearest candidates of every
    query row in float64, by (distance, index) -- numpy's stable argsort; None where a side is empty."""
    c = cloud_case(base)
    out = []
    for n in range(c.N):
        lx, ly = int(c.lx[n]), int(c.ly[n])
        if lx == 0 or ly == 0:
            out.append(None)
            continue
        q, t = c.p1[n, :lx].astype(np.float64), c.p2[n, :ly].astype(np.float64)
        order = np.empty((lx, min(KNN_MAX_K + 1, ly)), np.int64)
        dist = np.empty(order.shape)
        for a in range(0, lx, 64):                              # [64, l2] at a time
            d = ((q[a:a + 64, None, :] - t[None, :, :]) ** 2).sum(-1)
            o = np.argsort(d, axis=1, kind="stable")[:, :order.shape[1]]
            order[a:a + 64], dist[a:a + 64] = o, np.take_along_axis(d, o, 1)
        out.append((order, dist))
    return out


def upstream(name):
    """The random upstream gradient g [N,P1,K] of a case (float32)."""
    c, K = cloud_case(split(name)[0]), split(name)[1]
    return np.random.default_rng(77 + K).uniform(-1, 1, (c.N, c.P1, K)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(name):
    """float64: dists, idx [N,P1,K] (0 in invalid slots), valid [N,P1,K], hesitant rows [N,P1], the p2 rows they
    hesitate between [N,P2], and the gradients of sum(dists * upstream(name))."""
    base, K = split(name)
    c = cloud_case(base)
    dists, idx = np.zeros((c.N, c.P1, K)), np.zeros((c.N, c.P1, K), np.int64)
    valid = np.zeros((c.N, c.P1, K), bool)
    hes, skip2 = np.zeros((c.N, c.P1), bool), np.zeros((c.N, c.P2), bool)
    g1, g2 = np.zeros((c.N, c.P1, 3)), np.zeros((c.N, c.P2, 3))
    g = upstream(name).astype(np.float64)
    for n, so in enumerate(_sorted64(base)):
        if so is None:
            continue
        order, dist = so
        lx, ly = order.shape[0], int(c.ly[n])
        kv, m = min(K, ly), min(K + 1, ly)
        idx[n, :lx, :kv], dists[n, :lx, :kv], valid[n, :lx, :kv] = order[:, :kv], dist[:, :kv], True
        t32 = c.p2[n]
        a, b = order[:, :m - 1], order[:, 1:m]                   # consecutive entries
        close = (dist[:, 1:m] - dist[:, :m - 1]) <= TIE_GAP * dist[:, 1:m]
        close &= ~(t32[a] == t32[b]).all(-1)
        hes[n, :lx] = close.any(1)
        skip2[n, a[close]] = True
        skip2[n, b[close]] = True
        q, t = c.p1[n, :lx].astype(np.float64), c.p2[n, :ly].astype(np.float64)
        term = 2.0 * g[n, :lx, :kv, None] * (q[:, None, :] - t[order[:, :kv]])      # [lx, kv, 3]
        g1[n, :lx] = term.sum(1)
        np.add.at(g2[n], order[:, :kv].reshape(-1), -term.reshape(-1, 3))
    return dict(dists=dists, idx=idx, valid=valid, hesitant=hes, skip2=skip2, g1=g1, g2=g2)


def run_knn(name, device, fn=None):
    """The shim's knn_points on `device` with the case's upstream gradient -> (dists, idx, grad_p1, grad_p2) as numpy."""
    from acfm_video_3d_reconstruction_amd import pytorch3d_shim as p3d
    base, K = split(name)
    c = cloud_case(base)
    p1 = torch.tensor(c.p1, device=device, requires_grad=True)
    p2 = torch.tensor(c.p2, device=device, requires_grad=True)
    l1 = None if c.l1 is None else torch.tensor(c.l1, device=device)
    l2 = None if c.l2 is None else torch.tensor(c.l2, device=device)
    out = (fn or p3d.ops.knn_points)(p1, p2, l1, l2, K=K)
    dists, idx = out[0], out[1]
    assert dists.shape == idx.shape == (c.N, c.P1, K) and dists.dtype == torch.float32 and idx.dtype == torch.int64
    assert not idx.requires_grad
    dists.backward(torch.tensor(upstream(name), device=device))
    return dists.detach().cpu().numpy(), idx.cpu().numpy(), p1.grad.cpu().numpy(), p2.grad.cpu().numpy()


@functools.lru_cache(maxsize=None)
def host(name):
    return run_knn(name, torch.device("cpu"))


def check_forward(what, dists, idx, name):
    """Every bar on dists / idx (module docstring)."""
    base, K = split(name)
    c, r = cloud_case(base), reference(name)
    valid = r["valid"]
    assert np.isfinite(dists).all(), what
    assert not dists[~valid].any() and not idx[~valid].any(), "%s: an invalid slot is not 0 / 0" % what
    ly = np.asarray(c.ly)[:, None, None]
    assert ((idx >= 0) & (idx < np.maximum(ly, 1)))[valid].all(), "%s: an index outside [0, l2)" % what
    worst_ref = worst_own = 0.0
    for n in range(c.N):
        lx, kv = int(c.lx[n]), min(K, int(c.ly[n]))
        if lx == 0 or kv == 0:
            continue
        d, i = dists[n, :lx, :kv].astype(np.float64), idx[n, :lx, :kv]
        assert (np.diff(d, axis=1) >= 0).all(), "%s: dists not ascending" % what
        assert (np.diff(np.sort(i, 1), axis=1) > 0).all(), "%s: an index twice in a row" % what
        q, t = c.p1[n, :lx].astype(np.float64), c.p2[n].astype(np.float64)
        own = ((q[:, None, :] - t[i]) ** 2).sum(-1)              # recomputed from the returned index
        ref = r["dists"][n, :lx, :kv]
        for tag, want in (("reference", ref), ("own index", own)):
            np.testing.assert_allclose(d, want, rtol=DIST_RTOL, atol=0, err_msg="%s cloud %d vs %s" % (what, n, tag))
        worst_ref = max(worst_ref, float((np.abs(d - ref) / np.maximum(ref, 1e-300)).max()))
        worst_own = max(worst_own, float((np.abs(d - own) / np.maximum(own, 1e-300)).max()))
        dup = (c.p1[n, :lx, None, :] == c.p2[n][i]).all(-1)      # exact duplicates: exactly 0
        assert not dists[n, :lx, :kv][dup].any(), "%s: a duplicate at a distance other than 0" % what
        keep = ~r["hesitant"][n, :lx]
        bad = int((i != r["idx"][n, :lx, :kv])[keep].any(1).sum())
        assert bad == 0, "%s cloud %d: %d non-hesitant rows differ from the float64 order" % (what, n, bad)
    print("%s: dists rel err %.2e vs reference, %.2e vs own index (bar %.0e); %d hesitant rows left out"
          % (what, worst_ref, worst_own, DIST_RTOL, int(r["hesitant"].sum())))


def check_backward(what, g1, g2, name, host_grads=None):
    """Gradients on the kept rows; padded rows exactly 0.  host_grads: the host path's (grad_p1, grad_p2) for the L2
    bar (None: the floor alone, which is what the host path itself is held to)."""
    from test_shim_template_fit import REL_L2_FACTOR, REL_L2_FLOOR, _rel_l2, check_grad
    c, r = cloud_case(split(name)[0]), reference(name)
    for tag, got, ref, skip, P, lens, k in (("grad_p1", g1, r["g1"], r["hesitant"], c.P1, c.lx, 0),
                                            ("grad_p2", g2, r["g2"], r["skip2"], c.P2, c.ly, 1)):
        pad = np.arange(P)[None] >= np.asarray(lens)[:, None]
        assert not np.asarray(got)[pad].any(), "%s %s: padded rows must be exactly 0" % (what, tag)
        bar = REL_L2_FLOOR
        if host_grads is not None:
            bar = max(REL_L2_FLOOR, REL_L2_FACTOR * _rel_l2(host_grads[k], ref, ~skip))
        check_grad("%s %s" % (what, tag), got, ref, ~skip, bar)


# ============================================================================================ knn_gather
def gather_reference(x, idx, lengths):
    """float64 knn_gather: zeros where k >= lengths[n] or the index is outside [0, M) (the GPU contract)."""
    N, M, U = x.shape
    _, L, K = idx.shape
    ok = (idx >= 0) & (idx < M)
    if lengths is not None:
        ok &= np.arange(K)[None, None, :] < np.clip(lengths, 0, M)[:, None, None]
    out = x.astype(np.float64)[np.arange(N)[:, None, None], np.where(ok, idx, 0)]
    return np.where(ok[..., None], out, 0.0), ok


def gather_grad_reference(go, idx, ok, M):
    """index_add of grad_out [N,L,K,U] into [N,M,U] in float64, over the slots `ok`."""
    N, L, K, U = go.shape
    gx = torch.zeros((N, M, U), dtype=torch.float64)
    for n in range(N):
        sel = torch.from_numpy(ok[n].reshape(-1))
        gx[n].index_add_(0, torch.from_numpy(idx[n].reshape(-1).astype(np.int64))[sel],
                         torch.from_numpy(go[n].astype(np.float64)).reshape(-1, U)[sel])
    return gx.numpy()


# ============================================================================================ chamfer with normals
NORMAL_CASES = ["lengths", "ties", "n3-63x65"]        # chamfer_case names of tests/test_shim_template_fit.py
REDUCTIONS = [("sum", None, True), ("sum", "sum", False), ("mean", "mean", True), ("mean", "mean", False)]


@functools.lru_cache(maxsize=None)
def normals_case(name):
    """(x_normals, y_normals, clouds kept): unit normals in even clouds, normals of length 0.1 .. 3 in odd ones; a zero
    normal on each side of cloud 0 (cosine_similarity's eps branch); NaN at and past the lengths.  Kept: the clouds
    with both lengths > 0 (a length of 0 is 0 / 0 under point_reduction "mean")."""
    from test_shim_template_fit import chamfer_case
    c = chamfer_case(name)
    rng = np.random.default_rng(91 + c.P1)
    out = []
    for P, lens in ((c.P1, c.lx), (c.P2, c.ly)):
        nrm = rng.normal(size=(c.N, P, 3))
        nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
        nrm[1::2] *= rng.uniform(0.1, 3.0, (c.N, P, 1))[1::2]
        nrm = nrm.astype(np.float32)
        for n in range(c.N):
            nrm[n, int(lens[n]):] = np.nan
        out.append(nrm)
    out[0][0, min(2, c.P1 - 1)] = 0.0
    out[1][0, 1] = 0.0
    return out[0], out[1], [n for n in range(c.N) if c.lx[n] > 0 and c.ly[n] > 0]


def _pick(c, keep):
    sel = lambda a: None if a is None else a[keep]
    return c.x[keep], c.y[keep], sel(c.xl), sel(c.yl), c.w[keep]


@functools.lru_cache(maxsize=None)
def normals_reference(name, pr, br, weighted):
    """float64: (loss_normals, grad x_normals, grad y_normals) of sum(loss_normals), the neighbours taken from
    chamfer_reference (float64 argmin, lowest index); a point without a neighbour gathers a zero normal."""
    from test_shim_template_fit import chamfer_case, chamfer_reference
    c, r = chamfer_case(name), chamfer_reference(name)
    xn, yn, keep = normals_case(name)
    if pr == "sum" and br is None:
        keep = list(range(c.N))
    assert not r["tie_x"][keep].any() and not r["tie_y"][keep].any(), "a near tie picks another normal: choose another input"
    a = torch.tensor(np.nan_to_num(xn[keep]), dtype=torch.float64, requires_grad=True)
    b = torch.tensor(np.nan_to_num(yn[keep]), dtype=torch.float64, requires_grad=True)
    sums = []
    for own, other, idx, lens in ((a, b, r["ix"][keep], c.lx[keep]), (b, a, r["iy"][keep], c.ly[keep])):
        i = torch.from_numpy(idx)
        near = other.gather(1, i.clamp(min=0)[:, :, None].expand(-1, -1, 3))
        near = torch.where((i >= 0)[:, :, None], near, torch.zeros((), dtype=torch.float64))
        term = 1.0 - torch.nn.functional.cosine_similarity(own, near, dim=2, eps=1e-6).abs()
        live = torch.arange(own.shape[1])[None] < torch.from_numpy(np.asarray(lens))[:, None]
        s = torch.where(live, term, torch.zeros((), dtype=torch.float64)).sum(1)
        if weighted:
            s = s * torch.from_numpy(c.w[keep].astype(np.float64))
        if pr == "mean":
            s = s / torch.from_numpy(np.asarray(lens, np.float64))
        sums.append(s)
    total = sums[0] + sums[1]
    if br is not None:
        total = total.sum()
        if br == "mean":
            total = total / (float(c.w[keep].astype(np.float64).sum()) if weighted else float(len(keep)))
    total.sum().backward()
    return total.detach().numpy(), a.grad.numpy(), b.grad.numpy()


def run_normals(name, device, pr, br, weighted):
    """chamfer_distance with normals on `device` -> (loss, the loss without normals, loss_normals, grad x_normals,
    grad y_normals, grad x) as numpy; grad x is that of sum(loss_normals) alone: None, the index is an integer."""
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.loss import chamfer_distance
    from test_shim_template_fit import chamfer_case
    c = chamfer_case(name)
    xn, yn, keep = normals_case(name)
    if pr == "sum" and br is None:
        keep = list(range(c.N))
    x, y, xl, yl, w = _pick(c, keep)
    t = lambda a, grad=False: None if a is None else torch.tensor(a, device=device, requires_grad=grad)
    X, Y, XN, YN = t(x, True), t(y, True), t(xn[keep], True), t(yn[keep], True)
    kw = dict(x_lengths=t(xl), y_lengths=t(yl), weights=t(w) if weighted else None, batch_reduction=br, point_reduction=pr)
    loss, ln = chamfer_distance(X, Y, x_normals=XN, y_normals=YN, **kw)
    plain, none = chamfer_distance(X, Y, **kw)
    assert none is None
    gxn, gyn, gx = torch.autograd.grad(ln.sum(), [XN, YN, X], allow_unused=True)
    return (loss.detach().cpu().numpy(), plain.detach().cpu().numpy(), ln.detach().cpu().numpy(), gxn.cpu().numpy(),
            gyn.cpu().numpy(), gx)


@functools.lru_cache(maxsize=None)
def normals_host(name, pr, br, weighted):
    return run_normals(name, torch.device("cpu"), pr, br, weighted)


def check_normals(what, got, name, pr, br, weighted, host_run=None):
    from test_shim_template_fit import REL_L2_FACTOR, REL_L2_FLOOR, VALUE_RTOL, _rel_l2, check_grad
    loss, plain, ln, gxn, gyn, gx = got
    ref_v, ref_a, ref_b = normals_reference(name, pr, br, weighted)
    assert np.array_equal(loss, plain, equal_nan=True), "%s: the distance term changed its bits" % what
    assert gx is None, "%s: the points must get no gradient from the normal term" % what
    err = np.abs(ln - ref_v) / np.maximum(np.abs(ref_v), 1e-300)
    print("%s: loss_normals rel err %.2e (bar %.0e)" % (what, float(np.max(err)), VALUE_RTOL))
    np.testing.assert_allclose(ln, ref_v, rtol=VALUE_RTOL, atol=0, err_msg=what)
    for tag, g, r, k in (("grad x_normals", gxn, ref_a, 3), ("grad y_normals", gyn, ref_b, 4)):
        assert np.isfinite(g).all(), "%s %s" % (what, tag)
        bar = REL_L2_FLOOR
        if host_run is not None:
            bar = max(REL_L2_FLOOR, REL_L2_FACTOR * _rel_l2(host_run[k], r, np.ones(r.shape[:2], bool)))
        check_grad("%s %s" % (what, tag), g, r, np.ones(r.shape[:2], bool), bar)
