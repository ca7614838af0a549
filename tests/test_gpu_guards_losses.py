"""GPU: the loss unit (mask losses, texture MSE, boundary loss, optical-flow loss, the one-launch step tail, the
hypothesis total, the texture cycle, the visibility bitmap) on hostile, fenced memory: tests/guards.py run_case.

Bits are the claim wherever no float atomic is involved: every forward (the ticket finish sums its partials in a
fixed order) and the element-wise backwards.  The boundary loss's backward adds into LDS with float atomics, several
points per vertex, and has no deterministic mode: its gradient is held, in every run, to the float64 restatement and
the bars of tests/test_gpu_loss_shapes.py.  The optical-flow backward adds with global float atomics, but at T = 3 an
element gets at most two addends (the pair before and the pair after its frame) and a + b = b + a: bits there too."""
import numpy as np
import pytest
import torch

import guards
from test_gpu_loss_shapes import _bds_grad, _close, _first_min_argmin, _masks, _visibility_inputs

pytestmark = pytest.mark.gpu
_report = guards.module_report(__name__)

SIZES = [(17, 19), (40, 40)]


def _d():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, d, grad=False):
    return torch.tensor(a, device=d, requires_grad=grad)


def _reset():
    from acfm_video_3d_reconstruction_amd import ops
    ops.flush_pending_losses()
    guards._reset()


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("N,RB,with_gt,with_edt", [(6, 2, True, True), (3, 3, True, False), (3, 3, False, True)])
def test_mask_losses(H, W, N, RB, with_gt, with_edt):
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    rng = np.random.default_rng(H * 100 + N)
    mask, gt = _masks(rng, N, RB, H, W, "soft")
    edt = rng.uniform(0, 3, (RB, H, W)).astype(np.float32)
    w = rng.uniform(-1, 1, (N, 4)).astype(np.float32)

    def fn(inp):
        tm = inp(_t(mask, d, True))
        out = ops.mask_losses(tm, inp(_t(gt, d)) if with_gt else None, inp(_t(edt, d)) if with_edt else None)
        gm, = torch.autograd.grad((out * _t(w, d)).sum(), tm)
        return dict(out=out + 0, gm=gm + 0)          # (+ 0: a deferred term / an unformed gradient is formed in here)
    guards.run_case(fn, reset=_reset)


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("N,RB", [(6, 2), (3, 3)])
def test_tex_mse(H, W, N, RB):
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    rng = np.random.default_rng(H * 100 + N + 1)
    img = rng.uniform(0, 1, (RB, 3, H, W)).astype(np.float32)
    m = ((rng.uniform(size=(RB, H, W)) > 0.4) * rng.uniform(size=(RB, H, W))).astype(np.float32)
    tex = rng.uniform(0, 1, (N, 3, H, W)).astype(np.float32)
    w = rng.uniform(-1, 1, N).astype(np.float32)

    def fn(inp):
        tt = inp(_t(tex, d, True))
        out = ops.tex_mse(tt, inp(_t(img, d)), inp(_t(m, d)))
        gt, = torch.autograd.grad((out * _t(w, d)).sum(), tt)
        return dict(out=out + 0, gt=gt + 0)
    guards.run_case(fn, reset=_reset)


def _bds_inputs(V, P, N=4, RB=2):
    rng = np.random.default_rng(V * 1000 + P)
    xy = rng.uniform(-1, 1, (N, V, 2)).astype(np.float32)
    bds = np.concatenate([rng.uniform(-1, 1, (RB, P, 2)), np.ones((RB, P, 1))], -1).astype(np.float32)
    bds[:, max(1, (P * 4) // 5):, 2] = 0.0              # padding rows
    vis = (rng.uniform(size=(N, V)) > 0.3).astype(np.uint8)
    vis[0, rng.integers(V)] = 1
    vis[3] = 0                                           # nothing visible
    return xy, bds, vis, rng.uniform(0.5, 1.5, N)


@pytest.mark.parametrize("P", [63, 65])
@pytest.mark.parametrize("with_sel", [False, True])
def test_bds_loss(P, with_sel):
    """bds_loss_per_mesh at V = 65 without and with a slot list (drawn by boundary_subset: ascending slots, then -1):
    loss and argmin are bits; the gradient (LDS float atomics) against the float64 restatement in every run."""
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    V, N, RB = 65, 4, 2
    xy, bds, vis, w = _bds_inputs(V, P)
    S = 48
    state0 = torch.tensor([7, 0], dtype=torch.int64)
    counts = torch.tensor([P, P - 30], dtype=torch.int32)          # the second row: fewer slots than S -> a -1 tail

    def fn(inp):
        txy = inp(_t(xy, d, True))
        sel = ops.boundary_subset(state0.to(d), P, S, counts=counts.to(d), per_mesh=True) if with_sel else None
        loss = ops.bds_loss_per_mesh(txy, inp(_t(bds, d)), _t(vis, d), sel=sel)
        arg = loss.grad_fn.saved_tensors[3 if with_sel else 2] + 0      # (before the backward frees it)
        gxy, = torch.autograd.grad((loss * _t(w.astype(np.float32), d)).sum(), txy)
        loss = loss + 0
        if with_sel:             # the restatement on the selected points; an unselected slot weighs 0, like a padding point
            s = sel.cpu().numpy()
            assert s.shape == (RB, S) and (s[1] < 0).any() and (s[0] >= 0).all()
            sub = np.zeros((RB, S, 3), np.float32)
            for r in range(RB):
                sub[r, s[r] >= 0] = bds[r, s[r][s[r] >= 0]]
            live = np.stack([s[n % RB] >= 0 for n in range(N)])
        else:
            sub, live = bds, np.ones((N, P), bool)
        want = _first_min_argmin(xy, sub, vis, RB)
        np.testing.assert_array_equal(arg.cpu().numpy()[live], want[live])
        ref = _bds_grad(xy, sub, want, w, RB)
        _close(gxy, ref, what="bds gradient")
        out = dict(loss=loss, arg=arg, gxy=gxy)
        if with_sel:
            out["sel"] = sel
        return out
    guards.run_case(fn, reset=_reset, loose=("gxy",))


@pytest.mark.parametrize("H,W", SIZES)
def test_of_loss(H, W):
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    rng = np.random.default_rng(H)
    B, T, V, clips = 2, 3, 65, 1
    xy = rng.uniform(-1.1, 1.1, (B * T, V, 2))
    proj = np.concatenate([xy, rng.uniform(-1, 1, (B * T, V, 1))], -1).astype(np.float32)
    flows = rng.standard_normal((clips * T, H, W, 2)).astype(np.float32)
    masks = (rng.uniform(size=(clips * T, H, W)) > 0.25).astype(np.float32)
    vis = (rng.uniform(size=(B * T, V)) > 0.3).astype(np.uint8)
    w = rng.uniform(0.5, 1.5, (B, T - 1)).astype(np.float32)

    def fn(inp):
        tp = inp(_t(proj, d, True))
        loss = ops.of_loss(tp, inp(_t(flows, d)), _t(vis, d), B, T, masks=inp(_t(masks, d)), flip_t=True)
        count = loss.grad_fn.saved_tensors[3]
        gp, = torch.autograd.grad((loss * _t(w, d)).sum(), tp)
        return dict(loss=loss, count=count, gp=gp)
    plain, _ = guards.run_case(fn, reset=_reset)
    assert bool((plain["gp"] != 0).any())


@pytest.mark.parametrize("H,W", SIZES)
def test_combine_losses_over_deferred_terms(H, W):
    """mask_losses, tex_mse and bds_loss_per_mesh left pending and launched with the total by combine_losses
    (acfm_step_losses_forward), then the backward through all of them."""
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    rng = np.random.default_rng(W)
    N, RB, V, P = 4, 2, 65, 63
    mask, gt = _masks(rng, N, RB, H, W, "soft")
    edt = rng.uniform(0, 3, (RB, H, W)).astype(np.float32)
    img = rng.uniform(0, 1, (RB, 3, H, W)).astype(np.float32)
    tex = rng.uniform(0, 1, (N, 3, H, W)).astype(np.float32)
    xy, bds, vis, _ = _bds_inputs(V, P)
    weights = (1.0, 0.5, -0.25, 2.0, 3.0, 0.125)

    def fn(inp):
        tm, tt, txy = inp(_t(mask, d, True)), inp(_t(tex, d, True)), inp(_t(xy, d, True))
        a = ops.mask_losses(tm, inp(_t(gt, d)), inp(_t(edt, d)))
        b = ops.tex_mse(tt, inp(_t(img, d)), inp(_t(gt, d)))
        c = ops.bds_loss_per_mesh(txy, inp(_t(bds, d)), _t(vis, d))
        pending = [type(t) is ops.PendingTerm for t in (a, b, c)]
        total = ops.combine_losses([a, b, c], weights)
        gm, gt_, gxy = torch.autograd.grad(total, (tm, tt, txy))
        want = _first_min_argmin(xy, bds, vis, RB)
        _close(gxy, _bds_grad(xy, bds, want, np.full(N, weights[5] / N), RB), what="bds gradient through the total")
        return dict(total=total, a=a + 0, b=b + 0, c=c + 0, gm=gm + 0, gt=gt_ + 0, gxy=gxy,
                    pending=torch.tensor(pending))
    plain, _ = guards.run_case(fn, reset=_reset, loose=("gxy",))
    assert bool(plain["pending"].all()), "the terms were not deferred: the one-launch step tail did not run"


def test_hypothesis_total():
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    rng = np.random.default_rng(3)
    G, N = 3, 5
    terms = [rng.uniform(0, 1, (G * N,)).astype(np.float32) for _ in range(3)]

    def fn(inp):
        ts = [inp(_t(t, d, True)) for t in terms]
        out = ops.hypothesis_total(ts, (1.0, 0.5, 2.0), G, N, aux_group=(0, 1, -1), aux_weights=(1.0, 2.0, 0.0))
        gs = torch.autograd.grad(out[0], ts)
        return dict(weighted=out[0], total=out[1], probs=out[2], aux=out[3], means=out[4],
                    **{"g%d" % i: g for i, g in enumerate(gs)})
    guards.run_case(fn, reset=_reset)


def test_texture_cycle():
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    B, T, F, R = 2, 3, 65, 2
    tex = np.random.default_rng(4).uniform(0, 1, (B * T, F, R, R, 3)).astype(np.float32)

    def fn(inp):
        tt = inp(_t(tex, d, True))
        loss = ops.texture_cycle(tt, T)
        g, = torch.autograd.grad(loss, tt)
        return dict(loss=loss, g=g)
    guards.run_case(fn, reset=_reset)


def test_visible_vertices_stand_alone():
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    rng = np.random.default_rng(5)
    N, V = 3, 65
    vis = (rng.uniform(size=(N, V)) > 0.3).astype(np.uint8)
    faces, p2f = _visibility_inputs(rng, N, V, vis)

    def fn(inp):
        return dict(vis=ops.visible_vertices(torch.from_numpy(p2f).to(d), torch.from_numpy(faces).to(d), V))
    plain, _ = guards.run_case(fn, reset=_reset)
    np.testing.assert_array_equal(plain["vis"].cpu().numpy(), vis)
