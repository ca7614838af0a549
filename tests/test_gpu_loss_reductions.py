"""GPU: the per-mesh loss sums in one launch (acfm_mask_losses, acfm_tex_mse, acfm_bds_loss given tickets; behind
ops.mask_losses, ops.tex_mse and ops.bds_loss_per_mesh) -- every workgroup hands its partial sums over in a
persistent scratch, the one that draws a mesh's last ticket adds them in workgroup order.  Checked here: the same
bits on every call, values against the float64 references at the tolerances of test_gpu_loss_shapes.py, the ticket
words back at zero after every launch (same scratch again, then another shape on it), a captured graph replayed
three times, and the boundary loss bit for bit against what the library before this change answered
(tests/golden/bds_parent.npz, recorded by tools/record_bds_parent.py)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle import oracle as O
from test_gpu_loss_shapes import TOL, _first_min_argmin, _masks, _visibility_inputs

pytestmark = pytest.mark.gpu

MASK, TEX, BDS = 0, 1, 2


def _d():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _inputs(rng, N, RB, H, W, P, V, nothing_visible=True):
    mask, gt = _masks(rng, N, RB, H, W, "soft")
    edt = rng.uniform(0, 3, (RB, H, W)).astype(np.float32)
    img = rng.uniform(0, 1, (RB, 3, H, W)).astype(np.float32)
    m = ((rng.uniform(size=(RB, H, W)) > 0.4) * rng.uniform(size=(RB, H, W))).astype(np.float32)
    tex = rng.uniform(0, 1, (N, 3, H, W)).astype(np.float32)
    xy = rng.uniform(-1, 1, (N, V, 2)).astype(np.float32)
    bds = np.concatenate([rng.uniform(-1, 1, (RB, P, 2)), rng.uniform(size=(RB, P, 1)) > 0.1], -1).astype(np.float32)
    vis = (rng.uniform(size=(N, V)) > 0.45).astype(np.uint8)
    vis[0, rng.integers(V)] = 1
    if nothing_visible:
        vis[N - 1] = 0
    return dict(mask=mask, gt=gt, edt=edt, img=img, m=m, tex=tex, xy=xy, bds=bds, vis=vis)


def _to(d, x):
    return {k: torch.from_numpy(v).to(d) for k, v in x.items()}


def _three(t):
    """The three losses through the operators: ([N,4], [N], [N], argmin [N,P])."""
    from acfm_video_3d_reconstruction_amd import ops
    a = ops.mask_losses(t["mask"], t["gt"], t["edt"])
    b = ops.tex_mse(t["tex"], t["img"], t["m"])
    xy = t["xy"].detach().requires_grad_(True)
    c = ops.bds_loss_per_mesh(xy, t["bds"], t["vis"])
    return a, b, c.detach(), c.grad_fn.saved_tensors[2]


# (N, ref_batch, H, W, P, V): the headline shape, odd H*W (scalar branch), non-square, one mesh, 130 meshes (several
# grid rows, shared references), P = 1 .. 1537, V up to 2562.  The image kernels take 8192 pixels per workgroup once
# N * ceil(HW / 8192) >= 512: the headline shape (a multiple of 8192), and 130 meshes at 161 x 161 (odd H*W: the
# scalar branch, a partial last workgroup) and at 160 x 168 (vectorised, a partial last workgroup).
SHAPES = [(64, 64, 256, 256, 800, 642), (6, 2, 33, 33, 1, 5), (6, 3, 40, 72, 63, 65), (1, 1, 45, 91, 65, 642),
          (130, 65, 37, 53, 1000, 63), (4, 2, 97, 97, 1537, 2562), (130, 130, 64, 64, 129, 3),
          (130, 65, 161, 161, 70, 37), (130, 130, 160, 168, 5, 9)]


@pytest.mark.parametrize("N,RB,H,W,P,V", SHAPES)
def test_same_inputs_same_bits_and_float64_values(N, RB, H, W, P, V):
    """Each loss called twice (and a third time) on the same inputs: identical bits; and the values against the
    float64 references of test_gpu_loss_shapes.py at its tolerances."""
    d = _d()
    rng = np.random.default_rng(N * 7 + H * 1000 + W + P)
    x = _inputs(rng, N, RB, H, W, P, V)
    t = _to(d, x)
    first = _three(t)
    for _ in range(2):
        again = _three(t)
        for a, b in zip(first, again):
            assert torch.equal(a, b)
    what = str((N, RB, H, W, P, V))
    idx = np.arange(N) % RB
    f64 = lambda a: torch.tensor(a, dtype=torch.float64)
    rm, rg, re = f64(x["mask"]), f64(x["gt"][idx]), f64(x["edt"][idx])
    m2, g2 = rm.reshape(N, -1), rg.reshape(N, -1)
    ref = torch.stack([O.l1_loss(rm, rg, reduce=False), (m2 * g2).sum(1), (m2 + g2 - m2 * g2).sum(1),
                       O.edt_loss(rm, re[:, None], reduce=False)], 1)
    np.testing.assert_allclose(first[0].cpu().numpy(), ref.numpy(), err_msg=what, **TOL)
    ref = O.masked_texture_mse(f64(x["tex"]), f64(x["img"][idx]), f64(x["m"][idx]))
    np.testing.assert_allclose(first[1].cpu().numpy(), ref.numpy(), err_msg=what, **TOL)
    faces, p2f = _visibility_inputs(rng, N, V, x["vis"])
    ref = O.bds_loss(f64(x["xy"]), f64(x["bds"][idx]), torch.from_numpy(faces), torch.from_numpy(p2f), reduce=False)
    np.testing.assert_allclose(first[2].cpu().numpy(), ref.numpy(), err_msg=what, **TOL)
    np.testing.assert_array_equal(first[3].cpu().numpy(), _first_min_argmin(x["xy"], x["bds"], x["vis"], RB), err_msg=what)
    assert np.all(first[3][N - 1].cpu().numpy() == -1)


def _c_three(lib, t, N, RB, HW, P, V, scratch):
    """The three losses through the C ABI on caller-owned (tickets, partials) (None: the zero-fill + atomics form)."""
    from acfm_video_3d_reconstruction_amd import _lib
    d = t["mask"].device
    st = _lib.cur_stream(d)
    p = _lib.ptr
    a = torch.full((N, 4), 7.0, device=d)          # stale contents: the outputs need no prior zero
    b = torch.full((N,), 7.0, device=d)
    c = torch.full((N,), 7.0, device=d)
    arg = torch.empty((N, P), dtype=torch.int32, device=d)
    tk, part = scratch if scratch is not None else (None, None)
    nf = part.numel() if part is not None else 0
    _lib.check(lib.acfm_mask_losses(p(t["mask"]), p(t["gt"]), p(t["edt"]), N, HW, RB, p(a), p(tk), p(part), nf, st), "mask")
    _lib.check(lib.acfm_tex_mse(p(t["tex"]), p(t["img"]), p(t["m"]), N, HW, RB, p(b), p(tk), p(part), nf, st), "tex")
    _lib.check(lib.acfm_bds_loss(p(t["xy"]), p(t["bds"]), p(t["vis"]), None, N, V, P, RB, 0, 0, p(c), p(arg), p(tk), p(part),
                                 nf, st), "bds")
    return a, b, c, arg


def test_tickets_reset_themselves_on_one_scratch():
    """One set of zeroed ticket words and one partials buffer for all three losses: three back-to-back rounds, then
    another (N, HW, P), then the first shape again -- every result equals the first round's bits and the plain entry
    points' values, and the ticket words read zero after each round (the partials are left dirty on purpose).
    Too small a partials buffer and a missing pointer are refused."""
    from acfm_video_3d_reconstruction_amd import _lib
    d = _d()
    lib = _lib.lib()
    rng = np.random.default_rng(5)
    shapes = [(64, 64, 128, 128, 800, 642), (7, 7, 45, 91, 1537, 65)]
    need = max(int(lib.acfm_loss_partial_floats(w, N, n)) for N, _, H, W, P, _ in shapes
               for w, n in ((MASK, H * W), (TEX, H * W), (BDS, P)))
    assert int(lib.acfm_loss_partial_floats(MASK, 64, 128 * 128)) == 4 * 64 * 8
    assert int(lib.acfm_loss_partial_floats(TEX, 64, 128 * 128)) == 64 * 8
    assert int(lib.acfm_loss_partial_floats(BDS, 3, 70)) == 3 * 2
    assert int(lib.acfm_loss_partial_floats(3, 3, 70)) == 0 and int(lib.acfm_loss_partial_floats(MASK, 0, 70)) == 0
    tickets = torch.zeros(64, dtype=torch.int32, device=d)
    partials = torch.full((need,), float("nan"), device=d)
    data = [(_to(d, _inputs(rng, N, RB, H, W, P, V)), N, RB, H * W, P, V) for N, RB, H, W, P, V in shapes]
    firsts = {}
    for i in (0, 0, 0, 1, 0, 1):
        t, N, RB, HW, P, V = data[i]
        got = _c_three(lib, t, N, RB, HW, P, V, (tickets, partials))
        torch.cuda.synchronize()
        assert int(tickets.abs().max()) == 0, "ticket words left non-zero"
        if i not in firsts:
            firsts[i] = got
            plain = _c_three(lib, t, N, RB, HW, P, V, None)
            for a, b in zip(got[:3], plain[:3]):
                np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=2e-6, atol=1e-7)
            assert torch.equal(got[3], plain[3])
        for a, b in zip(got, firsts[i]):
            assert torch.equal(a, b)
    t, N, RB, HW, P, V = data[0]
    o = torch.empty((N, 4), device=d)
    args = (_lib.ptr(t["mask"]), _lib.ptr(t["gt"]), _lib.ptr(t["edt"]), N, HW, RB, _lib.ptr(o))
    assert lib.acfm_mask_losses(*args, _lib.ptr(tickets), _lib.ptr(partials), 4 * 64 * 8 - 1, _lib.cur_stream(d)) == 3
    assert lib.acfm_mask_losses(*args, None, _lib.ptr(partials), need, _lib.cur_stream(d)) == 1
    assert lib.acfm_mask_losses(*args, _lib.ptr(tickets), None, need, _lib.cur_stream(d)) == 1


def test_captured_graph_of_the_three_losses_replays_to_the_eager_bits():
    """All three losses in one captured graph, replayed three times (and once more on changed inputs): equal to the
    eager results bit for bit (the replay on changed inputs reads partial sums that the replay before wrote with
    other values: a stale read would show); the capture takes its ticket words from the zeroed chunk, so no fill is
    recorded with it."""
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    rng = np.random.default_rng(9)
    N, RB, H, W, P, V = 16, 8, 96, 80, 300, 642
    t = _to(d, _inputs(rng, N, RB, H, W, P, V))
    eager = _three(t)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _three(t)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _three(t)
    for _ in range(3):
        ops.graph_replay(graph)
        torch.cuda.synchronize()
        for a, b in zip(out, eager):
            assert torch.equal(a, b)
    t["mask"].mul_(0.5)
    t["tex"].mul_(0.25)
    t["xy"].mul_(0.5)
    ops.graph_replay(graph)
    torch.cuda.synchronize()
    for a, b in zip(out, _three(t)):
        assert torch.equal(a, b)
    assert not torch.equal(out[0], eager[0])


def test_two_streams_do_not_share_a_scratch():
    """The same loss in flight on two streams at once: each stream has its own slice of the pool, and both get the
    single-stream bits."""
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    rng = np.random.default_rng(13)
    t = _to(d, _inputs(rng, 64, 64, 256, 256, 800, 642))
    want = _three(t)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    got = []
    for _ in range(4):
        for s in (s1, s2):
            with torch.cuda.stream(s):
                got.append(_three(t))
    torch.cuda.synchronize()
    for g in got:
        for a, b in zip(g, want):
            assert torch.equal(a, b)
    keys = {k[1] for k in ops._LOSS_SCRATCH if k[1] in (s1.cuda_stream, s2.cuda_stream)}
    assert len(keys) == 2
    assert ops.loss_tickets_clean()


def test_boundary_loss_is_bit_equal_to_the_recorded_parent():
    """argmin and loss of the boundary loss == tests/golden/bds_parent.npz (the library before the visible-vertex
    staging and the ticket finish, tools/record_bds_parent.py) on grid inputs full of exact distance ties, with a
    mesh that has one visible vertex and one that has none: through the operator and through the plain entry point."""
    from acfm_video_3d_reconstruction_amd import _lib, ops
    d = _d()
    g = dict(np.load(os.path.join(GOLDEN, "bds_parent.npz")))
    n_cases = len([k for k in g if k.endswith("_xy")])
    assert n_cases >= 4
    ties = 0
    for i in range(n_cases):
        xy = g["c%d_xy" % i].astype(np.float32) / np.float32(16)
        b = np.concatenate([g["c%d_bd" % i].astype(np.float32) / np.float32(16),
                            g["c%d_flag" % i][..., None].astype(np.float32)], -1)
        vis, RB = g["c%d_vis" % i], int(g["c%d_rb" % i])
        N, V, _ = xy.shape
        P = b.shape[1]
        assert not vis[N - 1].any()
        txy, tb, tvis = torch.from_numpy(xy).to(d), torch.from_numpy(b).to(d), torch.from_numpy(vis).to(d)
        loss = ops.bds_loss_per_mesh(txy.requires_grad_(True), tb, tvis)
        arg = loss.grad_fn.saved_tensors[2]
        np.testing.assert_array_equal(arg.cpu().numpy(), g["c%d_argmin" % i], err_msg="case %d" % i)
        assert loss.detach().cpu().numpy().tobytes() == g["c%d_loss" % i].tobytes(), i
        l2 = torch.full((N,), -1.0, device=d)
        a2 = torch.empty((N, P), dtype=torch.int32, device=d)
        _lib.call("acfm_bds_loss", d, _lib.ptr(txy.detach()), _lib.ptr(tb), _lib.ptr(tvis), None, N, V, P, RB, 0, 0,
                  _lib.ptr(l2), _lib.ptr(a2), None, None, 0)
        np.testing.assert_array_equal(a2.cpu().numpy(), g["c%d_argmin" % i])
        assert l2.cpu().numpy().tobytes() == g["c%d_loss" % i].tobytes(), i
        assert np.all(g["c%d_argmin" % i][N - 1] == -1)
        # the inputs do hold exact ties: some point has two visible vertices at its least distance
        for n in range(N - 1):
            bb = b[n % RB]
            dd = ((bb[:, None, 0] - xy[n][None, :, 0]) ** 2 + (bb[:, None, 1] - xy[n][None, :, 1]) ** 2).astype(np.float32)
            dd[:, vis[n] == 0] = np.inf
            ties += int(((dd == dd.min(1, keepdims=True)).sum(1) > 1).sum())
    assert ties > 100
