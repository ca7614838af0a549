"""GPU: the step's tail as one launch (k_step_tail behind acfm_step_losses_forward).  ops.mask_losses, ops.tex_mse and
ops.bds_loss_per_mesh defer their launch and return ops.PendingTerm; ops.combine_losses launches the pending ones and
the total together.  The reference everywhere is the same call sequence under ops.defer_losses(False) -- the three
kernels and k_combine -- and every comparison is torch.equal: the roles run the bodies of those kernels on the same
partition with the same order of sums.

The shapes: N = 3 (one XCD group) and 8; H = 40, odd 57 (scalar loads, row tails, a last partial 16-byte piece) and 136;
P = 1, 64, 65, 1000; V = 642 and 12.  At these N the image roles take 2048 pixels per workgroup whatever H is
(8192 needs N * ceil(HW / 8192) >= 512), so one more case, 256 meshes at 96 x 96, runs the 8192-pixel form with a
partial last workgroup.  Every case has a mesh with an all-zero mask, a mesh with no visible vertex and non-finite
colours under zero texture-mask values."""
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

W4 = [1.0, 0.0, 0.0, 0.1]


def _d():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _inputs(N, H, P, V, RB=None, seed=0, half=False):
    RB = RB or N
    rng = np.random.default_rng(seed + N * 131 + H * 7 + P + V)
    HW = H * H
    mask = (rng.uniform(size=(N, H, H)) * (rng.uniform(size=(N, H, H)) > 0.6)).astype(np.float32)
    mask[1 % N] = 0.0                                           # an all-zero mask
    gt = (rng.uniform(size=(RB, H, H)) > 0.5).astype(np.float32)
    edt = rng.uniform(0, 3, (RB, H, H)).astype(np.float32)
    img = rng.uniform(0, 1, (RB, 3, H, H)).astype(np.float32)
    tex = rng.uniform(0, 1, (N, 3, H, H)).astype(np.float32)
    m = (rng.uniform(size=(RB, HW)) * (rng.uniform(size=(RB, HW)) > 0.4)).astype(np.float32)
    if not half:
        # aligned groups of four pixels with a zero texture mask, and non-finite colours under them: they must not
        # reach the sum (include/acfm_hip.h, acfm_tex_mse)
        dead = ((np.arange(HW) // 4) % 3 == 0)
        m[:, dead] = 0.0
        tex.reshape(N, 3, HW)[0][:, dead] = np.nan
        img.reshape(RB, 3, HW)[0][:, dead] = np.inf
    m = m.reshape(RB, H, H)
    xy = rng.uniform(-1, 1, (N, V, 2)).astype(np.float32)
    bds = np.concatenate([rng.uniform(-1, 1, (RB, P, 2)), rng.uniform(size=(RB, P, 1)) > 0.1], -1).astype(np.float32)
    vis = (rng.uniform(size=(N, V)) > 0.45).astype(np.uint8)
    vis[0, rng.integers(V)] = 1
    vis[N - 1] = 0                                              # a mesh with no visible vertex
    d = _d()
    t = {k: torch.from_numpy(v).to(d) for k, v in
         dict(mask=mask, gt=gt, edt=edt, img=img, tex=tex, m=m, xy=xy, bds=bds, vis=vis).items()}
    if half:
        for k in ("mask", "gt", "edt", "img", "tex", "m"):
            t[k] = t[k].half()
    return t


def _terms(t, roles, sel=None):
    from acfm_video_3d_reconstruction_amd import ops
    out = {}
    if "mask" in roles:
        out["mask"] = ops.mask_losses(t["mask"], t["gt"], t["edt"])
    if "bds" in roles:
        out["bds"] = ops.bds_loss_per_mesh(t["xy"], t["bds"], t["vis"], sel=sel)
    if "tex" in roles:
        out["tex"] = ops.tex_mse(t["tex"], t["img"], t["m"])
    return out


def _weights(roles):
    return [w for r in ("mask", "bds", "tex") if r in roles for w in {"mask": W4, "bds": [0.1], "tex": [0.5]}[r]]


def _run(t, roles, total=True, sel=None):
    """-> ({role: values}, argmin or None, total or None) with whatever deferral is in force."""
    from acfm_video_3d_reconstruction_amd import ops
    terms = _terms(t, roles, sel)
    order = [terms[r] for r in ("mask", "bds", "tex") if r in roles]
    tot = None
    if total:
        tot = ops.combine_losses(order, _weights(roles)).clone()
    else:
        ops.launch_pending_together(order)
    assert ops.loss_tickets_clean()
    return {r: v.detach().clone() for r, v in terms.items()}, tot


def _reference(t, roles, sel=None):
    from acfm_video_3d_reconstruction_amd import ops
    with ops.defer_losses(False):
        terms = _terms(t, roles, sel)
        assert not any(type(v) is ops.PendingTerm for v in terms.values())
        tot = ops.combine_losses([terms[r] for r in ("mask", "bds", "tex") if r in roles], _weights(roles))
    return {r: v.detach().clone() for r, v in terms.items()}, tot.clone()


def _same(got, ref, what):
    for r in ref[0]:
        assert torch.equal(got[0][r], ref[0][r]), "%s: term %s differs" % (what, r)
    if got[1] is not None:
        assert torch.equal(got[1], ref[1]), "%s: total differs (%r vs %r)" % (what, float(got[1]), float(ref[1]))


ALL = ("mask", "bds", "tex")
SHAPES = [(3, 40, 1, 12), (3, 57, 64, 642), (8, 40, 65, 642), (8, 57, 1000, 12), (3, 136, 1000, 642), (8, 136, 65, 12),
          (256, 96, 64, 12)]


@pytest.mark.parametrize("N,H,P,V", SHAPES)
def test_one_launch_equals_the_three_kernels_and_combine(N, H, P, V):
    from acfm_video_3d_reconstruction_amd import ops
    t = _inputs(N, H, P, V)
    ref = _reference(t, ALL)
    assert torch.isfinite(ref[1]), "non-finite colours under a zero mask reached the reference sum"
    terms = _terms(t, ALL)
    assert all(type(v) is ops.PendingTerm and v.is_pending for v in terms.values())
    tot = ops.combine_losses([terms[r] for r in ALL], _weights(ALL))
    assert not any(v.is_pending for v in terms.values())
    assert ops.loss_tickets_clean()
    _same(({r: v.detach() for r, v in terms.items()}, tot), ref, str((N, H, P, V)))
    # the argmin the backward reads
    with ops.defer_losses(False):
        a = ops.bds_loss_per_mesh(t["xy"].clone().requires_grad_(True), t["bds"], t["vis"])
    b = ops.bds_loss_per_mesh(t["xy"].clone().requires_grad_(True), t["bds"], t["vis"])
    ops.combine_losses([b], [0.1])
    assert torch.equal(a.grad_fn.saved_tensors[2], b.grad_fn.saved_tensors[2])
    # and a second launch on the same scratch
    _same(_run(t, ALL), ref, "again " + str((N, H, P, V)))


@pytest.mark.parametrize("roles", [("mask",), ("bds",), ("tex",), ("mask", "bds"), ("mask", "tex"), ("bds", "tex"), ALL])
@pytest.mark.parametrize("total", [True, False])
def test_role_subsets_with_and_without_total(roles, total):
    t = _inputs(3, 57, 65, 12, seed=1)
    _same(_run(t, roles, total=total), _reference(t, roles), "%s total=%s" % (roles, total))
    t = _inputs(8, 40, 64, 642, seed=2)
    _same(_run(t, roles, total=total), _reference(t, roles), "%s total=%s" % (roles, total))


def test_half_storage_inputs():
    t = _inputs(3, 40, 65, 12, seed=3, half=True)
    _same(_run(t, ALL), _reference(t, ALL), "half inputs")


def test_references_shared_by_two_hypotheses():
    t = _inputs(8, 57, 65, 642, RB=4, seed=4)
    _same(_run(t, ALL), _reference(t, ALL), "G = 2")
    t = _inputs(6, 40, 1000, 12, RB=3, seed=5)
    _same(_run(t, ALL), _reference(t, ALL), "G = 2")


def test_boundary_points_through_a_slot_list():
    t = _inputs(8, 40, 200, 642, RB=4, seed=6)
    sel = torch.full((4, 70), -1, dtype=torch.int32, device=_d())
    rng = np.random.default_rng(6)
    for r in range(4):
        k = [70, 64, 1, 0][r]
        sel[r, :k] = torch.from_numpy(np.sort(rng.choice(200, k, replace=False)).astype(np.int32))
    _same(_run(t, ALL, sel=sel), _reference(t, ALL, sel=sel), "slot list")
    _same(_run(t, ("bds",), sel=sel[:1].contiguous()), _reference(t, ("bds",), sel=sel[:1].contiguous()), "one list")


def test_a_term_no_role_writes_enters_the_total():
    from acfm_video_3d_reconstruction_amd import ops
    t = _inputs(8, 40, 65, 12, seed=7)
    prior = torch.rand(8, device=_d())
    with ops.defer_losses(False):
        a = ops.mask_losses(t["mask"], t["gt"], t["edt"])
        ref = ops.combine_losses([a, prior], W4 + [0.3])
    b = ops.mask_losses(t["mask"], t["gt"], t["edt"])
    assert torch.equal(ops.combine_losses([b, prior], W4 + [0.3]), ref)
    assert ops.loss_tickets_clean()


def _six_calls(t):
    from acfm_video_3d_reconstruction_amd import ops
    from acfm_video_3d_reconstruction_amd.nnutils import loss_utils as L
    sil4 = L.fused_silhouette_losses(t["mask"], t["gt"], t["edt"], raw=True)
    l1 = L.l1_loss(t["mask"], t["gt"], reduce=False)
    ed = L.edt_loss(t["mask"], t["edt"][:, None], reduce=False)
    bdt = ops.bds_loss_per_mesh(t["xy"], t["bds"], t["vis"])
    tm = L.masked_texture_mse(t["tex"], t["img"], t["m"])
    total = L.combine_losses([sil4, bdt, tm], W4 + [0.1, 0.5])
    return [x.detach() for x in (sil4, l1, ed, bdt, tm, total)]


def test_captured_sequence_replayed():
    from acfm_video_3d_reconstruction_amd import ops
    t = _inputs(8, 40, 65, 642, seed=8)
    eager = [x.clone() for x in _six_calls(t)]
    with ops.defer_losses(False):
        plain = _six_calls(t)
    for a, b in zip(eager, plain):
        assert torch.equal(a, b)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _six_calls(t)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        outs = _six_calls(t)
    for _ in range(3):
        for o in outs:
            o.fill_(-7.0)
        ops.graph_replay(g)
        torch.cuda.synchronize()
        for a, b in zip(outs, eager):
            assert torch.equal(a, b)
    assert ops.loss_tickets_clean()


def test_touching_a_term_first_gives_the_eager_value():
    from acfm_video_3d_reconstruction_amd import ops
    t = _inputs(3, 57, 65, 12, seed=9)
    ref = _reference(t, ALL)
    terms = _terms(t, ALL)
    assert torch.equal(terms["mask"].sum(), ref[0]["mask"].sum())
    assert not terms["mask"].is_pending and terms["bds"].is_pending and terms["tex"].is_pending
    tot = ops.combine_losses([terms[r] for r in ALL], _weights(ALL))
    _same(({r: v.detach() for r, v in terms.items()}, tot), ref, "touched first")
    assert ops.loss_tickets_clean()


def test_write_to_the_mask_before_the_launch_raises():
    from acfm_video_3d_reconstruction_amd import ops
    t = _inputs(3, 40, 65, 12, seed=10)
    sil4 = ops.mask_losses(t["mask"], t["gt"], t["edt"])
    t["mask"].mul_(0.5)
    with pytest.raises(RuntimeError, match="`mask`"):
        ops.combine_losses([sil4], W4)
    with pytest.raises(RuntimeError, match="`mask`"):
        sil4.sum()
    del sil4          # (the job goes with its term: nothing is left to launch)
    gc.collect()
    ops.flush_pending_losses()
    assert ops.loss_tickets_clean()


def test_gradients_of_the_whole_sequence(meshes):
    """verts, cams and atlas gradients of render -> losses -> total, deterministic backward: bit-equal with and without
    deferral."""
    from acfm_video_3d_reconstruction_amd import _lib, ops
    from acfm_video_3d_reconstruction_amd.nnutils import loss_utils as L
    from acfm_video_3d_reconstruction_amd.nnutils.nmr import NeuralRenderer
    from acfm_video_3d_reconstruction_amd.synthetic import batch_verts, make_cams
    d = _d()
    v, f = meshes["bird_v"], meshes["bird_f"]
    rng = np.random.default_rng(11)
    N, H, R, P = 3, 64, 2, 65
    verts0 = torch.tensor(batch_verts(v, N, rng), device=d)
    cams0 = torch.tensor(make_cams(N, rng, extent=float(np.abs(v).max())), device=d)
    faces = torch.from_numpy(f)[None].repeat(N, 1, 1).to(d)
    atlas0 = torch.tensor(rng.uniform(0, 1, (N, f.shape[0], R, R, 3)).astype(np.float32), device=d)
    gt = torch.tensor((rng.uniform(size=(N, H, H)) > 0.5).astype(np.float32), device=d)
    edt = torch.tensor(rng.uniform(0, 3, (N, 1, H, H)).astype(np.float32), device=d)
    img = torch.tensor(rng.uniform(0, 1, (N, 3, H, H)).astype(np.float32), device=d)
    ren = NeuralRenderer(H)
    # The boundary loss's backward adds the points of a vertex up with float atomics in LDS, in the order they arrive:
    # with three or more points on one vertex its bits change from run to run with or without deferral (two commute).
    # So every point here sits next to a visible vertex of its own (checked on the argmin below).
    with torch.no_grad():
        _, p2f0 = ren(verts0, faces, cams0)
        vis0 = ops.visible_vertices(p2f0, faces, v.shape[0]).cpu().numpy()
        xy0 = ops.project_xy(verts0, cams0, 0.).cpu().numpy()
    pts = np.stack([xy0[n][rng.choice(np.flatnonzero(vis0[n]), P, replace=False)] for n in range(N)]) + 2e-3
    bds = torch.tensor(np.concatenate([pts, np.ones((N, P, 1))], -1).astype(np.float32), device=d)

    def step():
        verts, cams, atlas = (x.clone().requires_grad_(True) for x in (verts0, cams0, atlas0))
        with _lib.raster_tuning(deterministic=True):
            mask, p2f = ren(verts, faces, cams)
            sil4 = L.fused_silhouette_losses(mask, gt, edt, raw=True)
            bdt = L.bds_loss(ren.project_points(verts, cams), bds, faces, p2f, reduce=False)
            tex, _, _ = ren(verts.detach(), faces, cams, textures=atlas)
            tm = L.masked_texture_mse(tex, img, gt)
            total = L.combine_losses([sil4, bdt, tm], W4 + [0.1, 0.5])
            arg = bdt.grad_fn.saved_tensors[2].cpu().numpy()
            assert max(np.bincount(a[a >= 0]).max() for a in arg) <= 2, "the test's boundary points share vertices"
            total.backward()
        return [total.detach(), verts.grad, cams.grad, atlas.grad]

    got = step()
    with ops.defer_losses(False):
        ref = step()
    for a, b, name in zip(got, ref, ("total", "verts", "cams", "atlas")):
        assert a is not None and torch.equal(a, b), name
    assert float(got[1].abs().max()) > 0 and float(got[2].abs().max()) > 0 and float(got[3].abs().max()) > 0
    assert ops.loss_tickets_clean()
