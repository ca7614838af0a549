"""GPU: the boundary-point draw on the device (acfm_sample.hip) against its numpy definition
(boundary_sampling.subset_host) index for index, the indexed boundary loss (k_bds_loss_sel / _bwd) against the CPU
oracle on the points a subset names, capture into a hipGraph, the drop-in surface (loss_utils.bds_loss(sampler=),
MultiframeStep(boundary_sampler=), ClipRefiner(boundary_sampler=)) and compute_boundaries(cap=)."""
import copy

import numpy as np
import pytest
import torch

from oracle import oracle as O

from acfm_video_3d_reconstruction_amd.boundary_sampling import BoundarySampler, draw_host

pytestmark = pytest.mark.gpu


def _d():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _state(s, d):
    seed, draw = s.state_on(d).cpu().tolist()
    return int(seed), int(draw)


# ------------------------------------------------------------------------------------------------ 1. the subset kernel
def _check_draws(P, n, counts=None, per_mesh=False, seed=11, ndraws=3):
    d = _d()
    s = BoundarySampler(n_samples=n, seed=seed, per_mesh=per_mesh)
    tc = None if counts is None else torch.tensor(counts, dtype=torch.int32, device=d)
    seen = []
    for t in range(ndraws):
        assert _state(s, d) == (seed, t)
        sel = s.draw(P, counts=tc, device=d)
        want = draw_host(seed, t, P, n, counts=counts, per_mesh=per_mesh)
        assert sel.dtype == torch.int32 and tuple(sel.shape) == want.shape
        np.testing.assert_array_equal(sel.cpu().numpy(), want, err_msg="P=%d n=%d counts=%s draw %d" % (P, n, counts, t))
        seen.append(want)
    assert _state(s, d) == (seed, ndraws)          # advanced by exactly one per call
    return seen


@pytest.mark.parametrize("P,n", [(1, 4), (7, 7), (8, 7), (64, 64), (65, 64), (1500, 1000), (4097, 64), (262144, 1000)])
def test_subset_kernel_equals_host_definition_shared(P, n):
    seen = _check_draws(P, n)
    if P > n:
        assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])


@pytest.mark.parametrize("counts,what", [([900, 1200, 7], "clip: the longest list is shorter than P"),
                                         ([1400, 5000, 3], "overflow: a count above P"),
                                         ([0, 0, 0], "all zero: the row is all -1")])
def test_subset_kernel_with_counts_shared(counts, what):
    seen = _check_draws(1500, 1000, counts=counts)
    k = min(1000, min(1500, max(counts)))
    assert int((seen[0] >= 0).sum()) == k, what
    if k:
        assert seen[0][0, :k].max() < min(1500, max(counts)), what


def test_subset_kernel_per_mesh():
    seen = _check_draws(1500, 1000, counts=[0, 5, 1500], per_mesh=True)
    assert (seen[0][0] == -1).all()
    np.testing.assert_array_equal(seen[0][1, :6], [0, 1, 2, 3, 4, -1])
    assert int((seen[0][2] >= 0).sum()) == 1000


def test_reseed_and_wide_state_words():
    """A negative seed and a draw counter past 2^32 (both words of both state entries are used), and reseed()."""
    d = _d()
    s = BoundarySampler(n_samples=64, seed=0)
    s.state_on(d)
    s.reseed(-7, draw=(1 << 32) + 5)
    sel = s.draw(4097, device=d)
    np.testing.assert_array_equal(sel.cpu().numpy(), draw_host(-7, (1 << 32) + 5, 4097, 64))
    assert _state(s, d) == (-7, (1 << 32) + 6)


# ------------------------------------------------------------------------------------------------ 2. the indexed loss
def _visibility_inputs(rng, N, V, vis, H=9, W=None):
    """One degenerate face (v, v, v) per vertex and a pix_to_face [N,H,W,1] that lists the packed ids of the visible
    vertices' faces: O.visible_vertices and ops.visible_vertices then give `vis`."""
    W = W or -(-V // H) + 2
    faces = np.repeat(np.arange(V, dtype=np.int64)[:, None], 3, 1)[None].repeat(N, 0)
    p2f = np.full((N, H * W, 1), -1, np.int64)
    for n in range(N):
        ids = np.nonzero(vis[n])[0]
        p2f[n, rng.permutation(H * W)[: ids.size], 0] = n * V + ids
    return faces, p2f.reshape(N, H, W, 1)


def _problem(V, N, RB, P, seed):
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-1, 1, (N, V, 2)).astype(np.float32)
    bds = np.concatenate([rng.uniform(-1, 1, (RB, P, 2)), (rng.uniform(size=(RB, P, 1)) > 0.1)], -1).astype(np.float32)
    vis = (rng.uniform(size=(N, V)) > 0.5).astype(np.uint8)       # about half the vertices
    vis[:, 0] = 1
    faces, p2f = _visibility_inputs(rng, N, V, vis)
    return rng, xy, bds, vis, faces, p2f


def _oracle_on_subset(xy, bds, faces, p2f, sel, w):
    """O.bds_loss (float64) on the points that sel names: (loss [N], d sum(w loss) / d xy)."""
    N, RB, rows = xy.shape[0], bds.shape[0], sel.shape[0]
    pts = np.zeros((N, sel.shape[1], 3), np.float64)
    for n in range(N):
        sl = sel[(n % RB) % rows]
        pts[n] = bds[n % RB][np.maximum(sl, 0)]
        pts[n, sl < 0, 2] = 0.0                                    # an empty entry adds nothing
    v = torch.tensor(xy, dtype=torch.float64, requires_grad=True)
    loss = O.bds_loss(v, torch.from_numpy(pts), torch.from_numpy(faces), torch.from_numpy(p2f), reduce=False)
    (loss * torch.from_numpy(w)).sum().backward()
    return loss.detach().numpy(), v.grad.numpy()


@pytest.mark.parametrize("V", [5, 642])
@pytest.mark.parametrize("RB", [4, 2])
@pytest.mark.parametrize("per_mesh", [False, True])
def test_indexed_loss_vs_oracle(V, RB, per_mesh):
    """ops.bds_loss_per_mesh(sel=) against O.bds_loss in float64 on the named points, at the tolerances of
    test_gpu_losses.py::test_bds_loss_golden_and_grad (loss rtol 1e-5 / atol 1e-5, gradient rtol 1e-4 / atol 1e-6)."""
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    N, P, n = 4, 1500, 1000
    rng, xy, bds, vis, faces, p2f = _problem(V, N, RB, P, seed=100 * V + 10 * RB + per_mesh)
    counts = [1500, 0, 1200, 700][:RB] if per_mesh else None      # per mesh: reference 1's row is all -1
    s = BoundarySampler(n_samples=n, seed=5, per_mesh=per_mesh)
    tc = None if counts is None else torch.tensor(counts, dtype=torch.int32, device=d)
    sel = s.draw(P, counts=tc, device=d)
    sel_h = draw_host(5, 0, P, n, counts=counts, per_mesh=per_mesh)
    np.testing.assert_array_equal(sel.cpu().numpy(), sel_h)
    if per_mesh:
        assert (sel_h[1] == -1).all()
    w = rng.uniform(0.5, 1.5, N)
    txy = torch.tensor(xy, device=d, requires_grad=True)
    tb, tv = torch.tensor(bds, device=d), torch.tensor(vis, device=d)
    loss = ops.bds_loss_per_mesh(txy, tb, tv, sel=sel)
    (loss * torch.tensor(w, device=d, dtype=torch.float32)).sum().backward()
    ref_loss, ref_grad = _oracle_on_subset(xy, bds, faces, p2f, sel_h, w)
    got = loss.detach().cpu().numpy()
    print("V=%d RB=%d per_mesh=%d: loss max rel err %.3g, grad max abs err %.3g (max |grad| %.3g)" % (
        V, RB, per_mesh, np.abs(got / np.maximum(ref_loss, 1e-30) - 1)[ref_loss > 0].max(),
        np.abs(txy.grad.cpu().numpy() - ref_grad).max(), np.abs(ref_grad).max()))
    np.testing.assert_allclose(got, ref_loss, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(txy.grad.cpu().numpy(), ref_grad, rtol=1e-4, atol=1e-6)
    if per_mesh:                                                   # meshes of the empty reference: exactly nothing
        for m in range(1, N, RB):
            assert got[m] == 0.0 and float(txy.grad[m].abs().max()) == 0.0
    # the forward is reproducible bit for bit
    again = ops.bds_loss_per_mesh(txy.detach(), tb, tv, sel=sel)
    assert torch.equal(again, loss.detach())


def test_indexed_loss_all_zero_counts():
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    _, xy, bds, vis, _, _ = _problem(642, 4, 2, 1500, seed=3)
    for per_mesh in (False, True):
        s = BoundarySampler(n_samples=1000, seed=1, per_mesh=per_mesh)
        sel = s.draw(1500, counts=torch.zeros(2, dtype=torch.int32, device=d))
        assert int(sel.max()) == -1
        txy = torch.tensor(xy, device=d, requires_grad=True)
        loss = ops.bds_loss_per_mesh(txy, torch.tensor(bds, device=d), torch.tensor(vis, device=d), sel=sel)
        loss.sum().backward()
        assert float(loss.detach().abs().max()) == 0.0 and float(txy.grad.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ 3. capture
def test_draw_loss_backward_in_a_hipgraph_redraws_every_replay():
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    N, V, RB, P, n = 4, 642, 4, 1500, 1000
    _, xy, bds, vis, _, _ = _problem(V, N, RB, P, seed=8)
    counts = [1500, 1300, 1100, 1450]
    for per_mesh in (False, True):
        s = BoundarySampler(n_samples=n, seed=21, per_mesh=per_mesh)
        tc = torch.tensor(counts, dtype=torch.int32, device=d)
        txy = torch.tensor(xy, device=d, requires_grad=True)
        tb, tv = torch.tensor(bds, device=d), torch.tensor(vis, device=d)

        def once():
            sel = s.draw(P, counts=tc)
            loss = ops.bds_loss_per_mesh(txy, tb, tv, sel=sel)
            loss.sum().backward()
            return sel, loss

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            once()                                               # state, scratch and allocator exist before the capture
        torch.cuda.current_stream().wait_stream(side)
        txy.grad = None
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            sel, loss = once()
        subsets = []
        for _ in range(3):
            seed, draw = _state(s, d)
            graph.replay()
            want = draw_host(seed, draw, P, n, counts=counts, per_mesh=per_mesh)
            np.testing.assert_array_equal(sel.cpu().numpy(), want)
            e_xy = txy.detach().clone().requires_grad_(True)
            eager = ops.bds_loss_per_mesh(e_xy, tb, tv, sel=torch.tensor(want, device=d))
            eager.sum().backward()
            assert torch.equal(loss.detach(), eager.detach())
            np.testing.assert_allclose(txy.grad.cpu().numpy(), e_xy.grad.cpu().numpy(), rtol=1e-4, atol=1e-6)
            assert _state(s, d) == (seed, draw + 1)
            subsets.append(want)
        assert not np.array_equal(subsets[0], subsets[1]) and not np.array_equal(subsets[1], subsets[2]) \
            and not np.array_equal(subsets[0], subsets[2])


# ------------------------------------------------------------------------------------------------ 4. drop-in surface
def test_loss_utils_surface():
    from acfm_video_3d_reconstruction_amd import ops
    from acfm_video_3d_reconstruction_amd.nnutils import loss_utils as L
    d = _d()
    N, V, RB, P, n = 4, 642, 4, 1500, 1000
    _, xy, bds, vis, faces, p2f = _problem(V, N, RB, P, seed=13)
    txy, tb, tv = torch.tensor(xy, device=d), torch.tensor(bds, device=d), torch.tensor(vis, device=d)
    tf, tp = torch.tensor(faces, device=d), torch.tensor(p2f, device=d)
    counts = torch.tensor([1500, 900, 1200, 1000], dtype=torch.int32, device=d)
    for per_mesh, cn in ((False, None), (False, counts), (True, counts)):
        s = BoundarySampler(n_samples=n, seed=2, per_mesh=per_mesh)
        for t, call in enumerate((lambda: L.bds_loss(txy, tb, tf, tp, reduce=False, sampler=s, counts=cn),
                                  lambda: L.Boundaries_Loss()(txy, tb, tf, tp, reduce=False, sampler=s, counts=cn))):
            got = call()
            want_sel = draw_host(2, t, P, n, counts=None if cn is None else cn.cpu().tolist(), per_mesh=per_mesh)
            want = ops.bds_loss_per_mesh(txy, tb, tv, sel=torch.tensor(want_sel, device=d))
            assert torch.equal(got, want)
        assert torch.equal(L.bds_loss(txy, tb, tf, tp, sampler=s, counts=cn),
                           ops.bds_loss_per_mesh(txy, tb, tv, sel=torch.tensor(
                               draw_host(2, 2, P, n, counts=None if cn is None else cn.cpu().tolist(), per_mesh=per_mesh),
                               device=d)).mean())
    with pytest.raises(NotImplementedError):
        L.bds_loss(txy, tb, tf, tp, k=2, sampler=BoundarySampler())
    # without a sampler and P <= 1000: today's path, the bits of the plain kernel on the same tensors
    small = tb[:, :1000].contiguous()
    assert torch.equal(L.bds_loss(txy, small, tf, tp, reduce=False), ops.bds_loss_per_mesh(txy, small, tv))


def test_multiframe_step_with_sampler_in_a_graphed_step(meshes):
    """MultiframeStep(boundary_sampler=) inside graphed.GraphedStep with 1500 boundary slots per frame (2 clips x 2
    frames, G = 2, 128^2): it constructs, replays twice, and the replayed loss equals the eager step's loss run from the
    same (seed, draw).  Bars: the first replay starts from identical parameters, inputs and subset, so only the
    summation order of fp32 reductions can differ: 1e-5 relative, the suite's bar for loss values; the second follows
    one optimiser step whose gradients carry float-atomic noise: 2e-3, the bar of
    test_gpu_losses.py::test_multiframe_step_hipgraph_matches_eager."""
    from acfm_video_3d_reconstruction_amd import image_utils as IU
    from acfm_video_3d_reconstruction_amd.graphed import GraphedStep
    from acfm_video_3d_reconstruction_amd.multiframe_step import MultiframeStep
    from acfm_video_3d_reconstruction_amd.synthetic import fps_lbs_logits, make_cams
    d = _d()
    torch.manual_seed(1)
    rng = np.random.default_rng(1)
    v, f = meshes["bird_v"], meshes["bird_f"]
    B, T, G, H, Kh = 2, 2, 2, 128, 15
    N = B * T
    sampler_g = BoundarySampler(n_samples=1000, seed=77, per_mesh=True)
    step_g = MultiframeStep(torch.tensor(v, device=d), torch.tensor(f, device=d),
                            torch.tensor(fps_lbs_logits(v, Kh), device=d), num_training_frames=10, img_size=H,
                            boundary_sampler=sampler_g, num_guesses=G, num_lbs=Kh, scale_lr_decay=1.0).to(d)
    step_e = copy.deepcopy(step_g)
    sampler_e = step_e.boundary_sampler = BoundarySampler(n_samples=1000, seed=77, per_mesh=True)
    gt_cams = torch.tensor(make_cams(N, rng, extent=float(np.abs(v).max())), device=d)
    with torch.no_grad():
        gt_mask, _ = step_g.renderer(step_g.solver.mean_v[None].repeat(N, 1, 1),
                                     step_g.faces1[None].expand(N, -1, -1), gt_cams)
        gt_mask = (gt_mask > 0.5).float()
    bds, counts = IU.compute_boundaries(gt_mask, cap=1500, return_counts=True)
    assert tuple(bds.shape) == (N, 1500, 3) and int(counts.min()) > 0

    def make_inputs(seed):
        g = torch.Generator(device="cpu").manual_seed(seed)
        return dict(masks=gt_mask, edts_barrier=IU.compute_dt(gt_mask, norm=False)[:, None].contiguous(),
                    boundaries=bds, boundary_counts=counts,
                    frames_idx=torch.randint(0, 10, (B, T), generator=g).to(d),
                    mirror_flag=torch.randint(0, 2, (N,), generator=g).to(d),
                    transforms=torch.tensor([[1., 0, 0, 0]] * N, device=d),
                    optical_flows=torch.randn(B, T, H, H, 2, generator=g).to(d),
                    delta=(0.01 * torch.randn(N, Kh, 3, generator=g)).to(d))

    fn = lambda step: (lambda i: step(i, i["delta"])[0])
    opt_g = torch.optim.SGD(step_g.parameters(), lr=1e-3, momentum=0.9)
    opt_e = torch.optim.SGD(step_e.parameters(), lr=1e-3, momentum=0.9)
    runner = GraphedStep(fn(step_g), opt_g, make_inputs(0), grad_inputs=("delta",))
    seed, draw = _state(sampler_g, d)
    assert seed == 77 and draw == 3                      # the warm-up iterations drew; the capture itself did not
    sampler_e.state_on(d)
    sampler_e.reseed(seed, draw)
    for it, bar in enumerate((1e-5, 2e-3)):
        inp = make_inputs(it)
        loss_g = runner(inp).item()
        opt_e.zero_grad(set_to_none=True)
        loss_e = fn(step_e)(inp)
        loss_e.backward()
        opt_e.step()
        print("replay %d: graph %.8g eager %.8g" % (it, loss_g, loss_e.item()))
        assert abs(loss_g - loss_e.item()) <= bar * abs(loss_e.item()), (it, loss_g, loss_e.item())
        assert _state(sampler_g, d) == _state(sampler_e, d) == (77, 4 + it)


def test_clip_refiner_with_sampler_captures_and_steps(meshes):
    from acfm_video_3d_reconstruction_amd import image_utils as IU, ops
    from acfm_video_3d_reconstruction_amd.deform import DeformSolver
    from acfm_video_3d_reconstruction_amd.nnutils.nmr import NeuralRenderer
    from acfm_video_3d_reconstruction_amd.refine import ClipRefiner
    from acfm_video_3d_reconstruction_amd.synthetic import fps_lbs_logits, make_cams
    d = _d()
    rng = np.random.default_rng(11)
    v, f = meshes["horse_v"], meshes["horse_f"]
    N, H, Kh = 4, 64, 8
    cams = torch.tensor(make_cams(N, rng, extent=float(np.abs(v).max())), device=d)
    faces = torch.tensor(f, device=d)[None].repeat(N, 1, 1).contiguous()
    solver = DeformSolver(torch.tensor(v, device=d), faces[0], torch.tensor(fps_lbs_logits(v, Kh), device=d))
    r = NeuralRenderer(H)
    with torch.no_grad():
        gt, _ = r(solver(torch.tensor(rng.normal(0, 0.05, (N, Kh, 3)).astype(np.float32), device=d)), faces, cams)
        gt = (gt > 0.5).float()
    edt = IU.compute_dt(gt, norm=False).reshape(N, 1, H, H).contiguous()
    bds, counts = IU.compute_boundaries(gt, cap=1500, return_counts=True)
    s = BoundarySampler(n_samples=1000, seed=4, per_mesh=True)
    ref = ClipRefiner(r, solver, torch.zeros(N, Kh, 3, device=d), cams, faces, gt, edt, bds, optimize_camera=True,
                      capturable=True, log_len=5, boundary_sampler=s, boundary_counts=counts)
    assert ref.capture(3) == 3 and _state(s, d) == (4, 3)
    ref.step()
    ref.step()
    assert _state(s, d) == (4, 5)
    hist = ref.history()
    assert len(hist) == 5 and all(np.isfinite(h) and h > 0 for h in hist)
    # every frame has fewer than 1000 boundary points here, so each draw takes them all: the loop is the one without
    # a sampler on the uncapped lists (the padding adds nothing) -- its first, eager, iteration to the fp32 sum order
    plain = ClipRefiner(r, solver, torch.zeros(N, Kh, 3, device=d), cams, faces, gt, edt,
                        IU.compute_boundaries(gt), optimize_camera=True, log_len=1)
    assert int(counts.max()) <= 1000
    plain.step()
    np.testing.assert_allclose(hist[0], plain.history()[0], rtol=1e-5)


# ------------------------------------------------------------------------------------------------ 5. compute_boundaries
def test_compute_boundaries_fixed_cap_and_counts():
    from acfm_video_3d_reconstruction_amd import image_utils as IU
    d = _d()
    H, W = 33, 20
    yy, xx = np.mgrid[:H, :W]
    masks = np.stack([np.zeros((H, W)), np.ones((H, W)), ((yy - 16) ** 2 + (xx - 9) ** 2 <= 49)]).astype(np.float32)
    tm = torch.tensor(masks, device=d)
    full = IU.compute_boundaries(tm)
    true_counts = full[..., 2].sum(1).to(torch.int32).cpu().numpy()
    longest = int(true_counts.max())
    assert full.shape[1] == longest and longest > 20 and true_counts[0] == 0 and true_counts[1] == 0
    for K in (longest + 7, longest // 2):
        out, counts = IU.compute_boundaries(tm, cap=K, return_counts=True)
        assert tuple(out.shape) == (3, K, 3) and counts.dtype == torch.int32 and counts.is_cuda
        np.testing.assert_array_equal(counts.cpu().numpy(), true_counts)
        assert torch.equal(IU.compute_boundaries(tm, cap=K), out)
        for b in range(3):
            k = min(int(true_counts[b]), K)
            assert torch.equal(out[b, :k], full[b, :k])
            pad = out[b, k:].cpu().numpy()
            assert (pad == np.array([-1.0, -1.0, 0.0], np.float32)).all()
    # the fixed-shape call makes no host read: it can be recorded into a hipGraph
    K = longest // 2
    static = tm.clone()
    IU.compute_boundaries(static, cap=K, return_counts=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, counts = IU.compute_boundaries(static, cap=K, return_counts=True)
    static.copy_(tm.flip(0))
    graph.replay()
    want, want_counts = IU.compute_boundaries(tm.flip(0), cap=K, return_counts=True)
    assert torch.equal(out, want) and torch.equal(counts, want_counts)
