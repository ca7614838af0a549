"""GPU: the kernels of csrc/acfm_lpips.hip through ops.lpips_* and perceptual.PerceptualTextureLoss against the literal
restatement of the spec (tests/lpips_literal.py) in float64.  Yardstick of every accuracy check (lpips_literal.check):
the error of the code under test may be at most twice that of the literal float32 torch composition, plus 1e-7 of the
largest reference magnitude.  Every figure is printed before it is asserted.  Inputs have no zero feature norm, except
in the test named for it."""
import pytest
import torch

import lpips_literal as L

pytestmark = pytest.mark.gpu


def _d():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _repeatable():
    """torch's convolutions with run-to-run reproducible algorithms: MIOpen's default choices for AlexNet's 3 x 3
    layers differ in the last bit from one run to the next, so a bit comparison of two runs of the whole loss says
    something about this package's part only with them pinned."""
    return torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True)


def _mask(n, H, W, gen):
    m = (torch.rand(n, H, W, generator=gen) > 0.4).float()
    m[:, : max(H // 4, 1)] = 0                       # empty rows
    return m


LAYER_SHAPES = [(2, 2, 64, 15, 15), (3, 3, 192, 7, 7), (2, 2, 384, 3, 3), (1, 1, 256, 1, 1), (2, 2, 5, 4, 4),
                (2, 2, 67, 9, 5), (6, 2, 64, 15, 15)]


# from 2048 tiles of 64 pixels on, the layer kernels run four waves per tile instead of sixteen: one shape on that path
WIDE_LAYER_SHAPE = (2, 2, 8, 256, 256)


@pytest.mark.parametrize("with_lin", [False, True], ids=["unit", "lin"])
@pytest.mark.parametrize("shape", LAYER_SHAPES + [WIDE_LAYER_SHAPE], ids=lambda s: "x".join(map(str, s)))
def test_layer_forward_backward(shape, with_lin):
    from acfm_video_3d_reconstruction_amd import ops
    N, Nr, C, h, w = shape
    g = _gen(sum(shape) + with_lin)
    a, b = L.features((N, C, h, w), g), L.features((Nr, C, h, w), g)
    lin = torch.rand(C, generator=g) if with_lin else None
    gd = torch.randn(N, h, w, generator=g)
    dev = _d()
    swap = Nr == N
    lit = {}
    for dt in (torch.float64, torch.float32):
        x = a.to(dev, dt).requires_grad_(True)
        y = b.to(dev, dt).requires_grad_(swap)
        dd = L.lit_layer(x, y.repeat(N // Nr, 1, 1, 1), lin.to(dev) if with_lin else None)[:, 0]
        lit[dt] = (dd.detach(),) + torch.autograd.grad(dd, [x, y] if swap else [x], gd.to(dev, dt))
    x = a.to(dev).requires_grad_(True)
    y = b.to(dev).requires_grad_(swap)
    d = ops.lpips_layer(x, y, lin.to(dev) if with_lin else None)
    grads = torch.autograd.grad(d, [x, y] if swap else [x], gd.to(dev))
    tag = "layer %s%s" % (shape, " lin" if with_lin else "")
    L.check(tag, d, lit[torch.float32][0], lit[torch.float64][0])
    L.check(tag + " grad a", grads[0], lit[torch.float32][1], lit[torch.float64][1])
    if swap:
        L.check(tag + " grad b (roles exchanged)", grads[1], lit[torch.float32][2], lit[torch.float64][2])


def test_layer_refuses_shared_reference_that_requires_grad():
    from acfm_video_3d_reconstruction_amd import ops
    g = _gen(1)
    a = L.features((6, 8, 3, 3), g).to(_d())
    b = L.features((2, 8, 3, 3), g).to(_d()).requires_grad_(True)
    with pytest.raises(ValueError, match="lpips_layer.*cannot require grad"):
        ops.lpips_layer(a, b)


def test_layer_zero_norm_pixels():
    """One all-zero a, one all-zero b, one both: u = 0 there; the gradient is finite and is
    q_c / (n_a + eps) - a_c (sum_k q_k a_k) / (n_a (n_a + eps)^2) with the second term 0 where n_a = 0."""
    from acfm_video_3d_reconstruction_amd import ops
    g = _gen(2)
    C = 67
    a, b = L.features((1, C, 2, 3), g), L.features((1, C, 2, 3), g)
    a[0, :, 0, 0] = 0
    b[0, :, 0, 1] = 0
    a[0, :, 0, 2] = 0
    b[0, :, 0, 2] = 0
    gd = torch.randn(1, 2, 3, generator=g)
    eps = 1e-10

    def formula(a, b, gd):          # the stated definition and gradient, on one dtype
        na, nb = (a * a).sum(1, keepdim=True).sqrt(), (b * b).sum(1, keepdim=True).sqrt()
        u, v = a / (na + eps), b / (nb + eps)
        d = ((u - v) ** 2).sum(1)
        q = 2 * (u - v) * gd[:, None]
        second = a * (q * a).sum(1, keepdim=True) / torch.where(na > 0, na * (na + eps) ** 2, torch.ones_like(na))
        return d, q / (na + eps) - torch.where(na > 0, second, torch.zeros_like(second))
    d64, g64 = formula(a.double(), b.double(), gd.double())
    d32, g32 = formula(a, b, gd)
    x = a.to(_d()).requires_grad_(True)
    d = ops.lpips_layer(x, b.to(_d()))
    ga, = torch.autograd.grad(d, x, gd.to(_d()))
    assert bool(torch.isfinite(ga).all())
    assert float(d.detach()[0, 0, 2]) == 0.0 and float(ga[0, :, 0, 2].abs().max()) == 0.0
    L.check("zero-norm forward", d, d32, d64)
    L.check("zero-norm gradient", ga, g32, g64)


@pytest.mark.parametrize("N,Nr,H,W", [(4, 2, 64, 64), (1, 1, 5, 7)])
def test_input_kernel(N, Nr, H, W):
    from acfm_video_3d_reconstruction_amd import ops
    g = _gen(3)
    img = torch.rand(N, 3, H, W, generator=g)
    mask = _mask(Nr, H, W, g)
    mask[0, -1] = 0.5                                   # a fractional row too
    rep = mask.repeat(N // Nr, 1, 1)
    gy = torch.randn(N, 3, H, W, generator=g)
    dev = _d()
    lit = {}
    for dt in (torch.float64, torch.float32):
        x = img.to(dev, dt).requires_grad_(True)
        y = L.lit_input(x, rep.to(dev, dt))
        lit[dt] = (y.detach(), torch.autograd.grad(y, x, gy.to(dev, dt))[0])
    x = img.to(dev).requires_grad_(True)
    y = ops.lpips_input(x, mask.to(dev))
    gx, = torch.autograd.grad(y, x, gy.to(dev))
    L.check("input %dx%d" % (H, W), y, lit[torch.float32][0], lit[torch.float64][0])
    L.check("input grad %dx%d" % (H, W), gx, lit[torch.float32][1], lit[torch.float64][1])
    assert float(gx[rep[:, None].expand_as(gx) == 0].abs().max()) == 0.0


@pytest.mark.parametrize("H,W,sizes", [(64, 64, [(15, 15), (7, 7), (3, 3), (3, 3), (3, 3)]),
                                       (40, 56, [(9, 13), (4, 6), (1, 2)])])
def test_mask_weights(H, W, sizes):
    """Against the host path (the float32 adjoint from autograd), both measured against the float64 adjoint."""
    import torch.nn.functional as F
    from acfm_video_3d_reconstruction_amd import ops
    g = _gen(4)
    Nr = 3
    mask = _mask(Nr, H, W, g)
    mask[1] = torch.rand(H, W, generator=g)              # a soft mask too
    host = ops.lpips_mask_weights(mask, sizes)
    m64 = mask.double()[:, None] / (H * W)
    M64 = []
    for h, w in sizes:
        z = torch.zeros(Nr, 1, h, w, dtype=torch.float64, requires_grad=True)
        up = F.interpolate(z, size=(H, W), mode="bilinear", align_corners=False)
        M64.append(torch.autograd.grad((up * m64).sum(), z)[0].reshape(Nr, -1))
    M = ops.lpips_mask_weights(mask.to(_d()), sizes)
    L.check("mask weights %dx%d" % (H, W), M, host, torch.cat(M64, 1))
    assert torch.equal(M, ops.lpips_mask_weights(mask.to(_d()), sizes))


def test_masked_mean():
    from acfm_video_3d_reconstruction_amd import _lib, ops
    g = _gen(5)
    N, Nr, P = 6, 2, 301
    d, M, gl = torch.rand(N, P, generator=g), torch.rand(Nr, P, generator=g) / P, torch.randn(N, generator=g)
    dev = _d()
    lit = {}
    for dt in (torch.float64, torch.float32):
        x = d.to(dev, dt).requires_grad_(True)
        l = (x * M.to(dev, dt).repeat(N // Nr, 1)).sum(1)
        lit[dt] = (l.detach(), torch.autograd.grad(l, x, gl.to(dev, dt))[0])
    x = d.to(dev).requires_grad_(True)
    loss = ops.lpips_masked_mean(x, M.to(dev))
    gd, = torch.autograd.grad(loss, x, gl.to(dev))
    L.check("masked mean", loss, lit[torch.float32][0], lit[torch.float64][0])
    L.check("masked mean grad", gd, lit[torch.float32][1], lit[torch.float64][1])
    assert torch.equal(loss, ops.lpips_masked_mean(x, M.to(dev)))
    # the output is written, not accumulated: a buffer full of NaN comes back clean
    out = torch.full((N,), float("nan"), device=dev)
    xd, Md = d.to(dev), M.to(dev)
    _lib.call("acfm_lpips_masked_mean_forward", dev, _lib.ptr(xd), _lib.ptr(Md), N, Nr, P, _lib.ptr(out))
    assert torch.equal(out, loss.detach())


@pytest.fixture(scope="module")
def whole():
    """N = 4, Nr = 2, 64 x 64, seeded random AlexNet weights: the float64 literal on the CPU (once), the float32 literal
    and the code under test on the GPU."""
    from acfm_video_3d_reconstruction_amd import perceptual
    g = _gen(6)
    N, Nr, H = 4, 2, 64
    sd = L.alex_state(0)
    pred, img = torch.rand(N, 3, H, H, generator=g), torch.rand(Nr, 3, H, H, generator=g)
    mask, gl = _mask(Nr, H, H, g), torch.rand(N, generator=g)
    G = N // Nr
    dev = _d()
    out = {}
    for dt, where in ((torch.float64, torch.device("cpu")), (torch.float32, dev)):
        x = pred.to(where, dt).requires_grad_(True)
        l = L.lit_loss(x, img.to(where, dt).repeat(G, 1, 1, 1), mask.to(where, dt).repeat(G, 1, 1),
                       {k: v.to(where) for k, v in sd.items()})
        out[dt] = (l.detach(), torch.autograd.grad(l, x, gl.to(where, dt))[0])
    fn = perceptual.PerceptualTextureLoss(perceptual.AlexFeatures(sd)).to(dev)
    return dict(fn=fn, pred=pred.to(dev), img=img.to(dev), mask=mask.to(dev), gl=gl.to(dev), lit=out)


def test_whole_loss(whole):
    fn = whole["fn"]
    x = whole["pred"].clone().requires_grad_(True)
    per = fn(x, whole["img"], None, whole["mask"], reduce=False)
    gp, = torch.autograd.grad(per, x, whole["gl"])
    lit = whole["lit"]
    L.check("whole loss", per, lit[torch.float32][0], lit[torch.float64][0])
    L.check("whole loss grad", gp, lit[torch.float32][1], lit[torch.float64][1])
    with _repeatable(), torch.no_grad():
        per = fn(whole["pred"], whole["img"], None, whole["mask"], reduce=False)
        assert torch.equal(fn(whole["pred"], whole["img"], None, whole["mask"]), per.mean())


def test_prepare_against_is_the_direct_call(whole):
    fn = whole["fn"]
    with _repeatable(), torch.no_grad():
        direct = fn(whole["pred"], whole["img"], None, whole["mask"], reduce=False)
        prepared = fn.prepare(whole["img"], whole["mask"])
        assert torch.equal(fn.against(prepared, whole["pred"], reduce=False), direct)
        assert torch.equal(fn.against(prepared, whole["pred"], reduce=False), direct)      # reused


def test_layers_and_masked_mean_captured():
    """ops.lpips_layers + ops.lpips_masked_mean, forward and backward, as one graph (the convolutions stay outside):
    replayed on changed inputs, it gives the eager results bit for bit."""
    from acfm_video_3d_reconstruction_amd import ops
    g = _gen(7)
    dev = _d()
    N, Nr = 4, 2
    shapes = [(64, 15, 15), (192, 7, 7), (384, 3, 3)]

    def draw():
        return ([L.features((N,) + s, g).to(dev) for s in shapes], [L.features((Nr,) + s, g).to(dev) for s in shapes],
                (torch.rand(Nr, sum(s[1] * s[2] for s in shapes), generator=g) / 300).to(dev),
                torch.randn(N, generator=g).to(dev))

    def run(fas, fbs, M, gl):
        xs = [a.requires_grad_(True) for a in fas]
        loss = ops.lpips_masked_mean(ops.lpips_layers(xs, fbs), M)
        return (loss.detach(),) + torch.autograd.grad(loss, xs, gl)
    fas, fbs, M, gl = draw()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(fas, fbs, M, gl)                               # eager warm-up
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run(fas, fbs, M, gl)
    fas2, fbs2, M2, gl2 = draw()
    want = [t.clone() for t in run([a.clone() for a in fas2], fbs2, M2, gl2)]
    with torch.no_grad():
        for dst, src in zip(fas + fbs + [M, gl], fas2 + fbs2 + [M2, gl2]):
            dst.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    for o, w in zip(outs, want):
        assert torch.equal(o, w)


def test_multiframe_step_perceptual_term(meshes):
    """MultiframeStep.forward(perceptual=...) adds 0.5 LPIPS + 0.5 LPIPS(flipped) (main.py:647-654) as one term of
    weight tex_loss_wt; it is off by default, and with it on the other terms keep their bits."""
    import numpy as np
    from acfm_video_3d_reconstruction_amd import image_utils as IU, ops, perceptual
    from acfm_video_3d_reconstruction_amd.multiframe_step import MultiframeStep
    from acfm_video_3d_reconstruction_amd.synthetic import fps_lbs_logits, make_cams
    d = _d()
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    v, f = meshes["bird_v"], meshes["bird_f"]
    B, T, G, H, Kh = 1, 2, 2, 64, 15
    N = B * T
    step = MultiframeStep(torch.tensor(v, device=d), torch.tensor(f, device=d),
                          torch.tensor(fps_lbs_logits(v, Kh), device=d), num_training_frames=4, img_size=H,
                          num_guesses=G, num_lbs=Kh, scale_lr_decay=1.0).to(d)
    gt_cams = torch.tensor(make_cams(N, rng, extent=float(np.abs(v).max())), device=d)
    with torch.no_grad():
        gt_mask, _ = step.renderer(step.solver.mean_v[None].repeat(N, 1, 1), step.faces1[None].expand(N, -1, -1), gt_cams)
        gt_mask = (gt_mask > 0.5).float()
    batch = dict(masks=gt_mask, edts_barrier=IU.compute_dt(gt_mask, norm=False)[:, None].contiguous(),
                 boundaries=IU.compute_boundaries(gt_mask), frames_idx=torch.tensor([[0, 1]], device=d),
                 mirror_flag=torch.tensor([0, 0], device=d), transforms=torch.tensor([[1., 0, 0, 0]] * N, device=d))
    delta = (0.01 * torch.randn(N, Kh, 3, device=d)).requires_grad_(True)
    tex = torch.rand(N, f.shape[0], 4, 4, 3, device=d, requires_grad=True)
    imgs = torch.rand(N, 3, H, H, device=d)
    fn = perceptual.PerceptualTextureLoss(perceptual.AlexFeatures(L.alex_state(0))).to(d)
    total0, terms0 = step(batch, delta, textures=tex, imgs=imgs)
    g0, = torch.autograd.grad(total0, tex)
    assert "tex_lpips" not in terms0
    total1, terms1 = step(batch, delta, textures=tex, imgs=imgs, perceptual=fn)
    g1, = torch.autograd.grad(total1, tex)
    for k in ("pred_v", "cam_pred", "mask_loss"):          # the terms whose bits repeat from run to run
        assert torch.equal(terms0[k], terms1[k]), k
    for k in ("mask", "sil_cons", "rigid", "triangle", "tex_mse", "tex_mse_per_hyp", "cycle"):
        # the same code on the same inputs; some of these sum with float atomics, whose order moves the last bits
        assert torch.allclose(terms0[k], terms1[k], rtol=1e-5, atol=0), k
    assert bool(torch.isfinite(g1).all()) and not torch.equal(g0, g1)
    # the term itself, from the renders of the same cameras and vertices
    with torch.no_grad():
        cam, pred_v = terms1["cam_pred"], terms1["pred_v"].repeat(G, 1, 1)
        faces = step.faces1[None].expand(G * N, -1, -1)
        t0, _, _ = step.tex_renderer(pred_v, faces, cam, textures=tex)
        t1, _, _ = step.tex_renderer(pred_v, faces, ops.camera_mirror(cam), textures=tex)
        want = 0.5 * fn(t0, imgs, None, gt_mask, reduce=False) \
            + 0.5 * fn(t1, imgs.flip(3), None, gt_mask.flip(2), reduce=False)
    print("tex_lpips %.8f, recomputed %.8f" % (float(terms1["tex_lpips"]), float(want.mean())))
    # two float32 evaluations whose convolutions may differ in the last bits (2.4e-7 on the taps): 1e-5 relative
    assert float(want.mean()) > 0 and abs(float(terms1["tex_lpips"]) - float(want.mean())) <= 1e-5 * float(want.mean())
