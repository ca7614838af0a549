"""GPU: the kernel variants the launch heuristics never pick at the tiny shapes of the rest of the suite
(tests/dispatch_cases.py names the cases, tests/test_dispatch_cases.py shows on the CPU that each sits on its branch):
  * k_dconv_fwd<*, 2> and <*, 4>: the 32- and 64-channel tiles of the deformable convolution;
  * k_dconv_bwd_weight with more than one pixel tile per workgroup, empty parts, the 1024-part cap, and a workgroup
    that goes from one image to the next;
  * k_correlation_fwd<2..4, false> with three LDS chunks and <1, true>;
  * k_lpips_layer_{fwd,bwd}<4> at odd C, shared references, tiles across images and a partial last tile, next to its
    sixteen-wave neighbour on nearly the same data;
  * k_phong_bwd<true, true> (flat shading, deterministic mode) and the shininess == 0 branch of the lit backward;
  * the atlas form of the softmax blend (k_softmax_blend_{fwd,bwd}<K, true, *>) at the with_k instantiations K = 2, 8,
    20 and 32, which the built-fragment tests run at K = 1, 4 and 10 only, in the default and the deterministic mode.
Every bar is the one the unit's own test file uses (imported from there); every figure is printed before it is
asserted."""
import numpy as np
import pytest
import torch

import dispatch_cases as dc
import guards
import lit_reference as R
import lpips_literal as L
from oracle import oracle as O
from test_flow_grad import BOUND, corr_ref_grads, dconv_ref_grads, draw_go, nudge, ratio
from test_flow_ops import TOL, make_inputs, tile9
from test_gpu_flow_grad import _corr_grads, _dconv_grads
from test_gpu_lit_shading import _check_shade, _leaf, _light, _shade_case, _sphere
from test_gpu_shader_fragments import ATLAS_CASES, FRAGMENT_K
from test_gpu_shader_fragments import test_atlas_texels as _atlas_texels

pytestmark = pytest.mark.gpu
_ID = lambda c: "x".join(str(v) for v in c)


def _d():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _lib():
    from acfm_video_3d_reconstruction_amd import _lib
    return _lib.lib()


def _allclose(name, got, ref):
    """np.testing.assert_allclose at TOL, with the worst error as a share of the tolerance printed first."""
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else got
    share = np.abs(got - ref) / (TOL["atol"] + TOL["rtol"] * np.abs(ref))
    print("%s: worst error %.3f of the tolerance, max |got - ref| %.3g" % (name, share.max(), np.abs(got - ref).max()))
    np.testing.assert_allclose(got, ref, **TOL)


def _ratio(name, got, ref):
    r = ratio(got.detach().cpu().numpy() if torch.is_tensor(got) else got, ref)
    print("%s: max|got - ref| / max|ref| = %.3e" % (name, r))
    assert r <= BOUND, (name, r)


# ------------------------------------------------------------------------------ deformable convolution, forward
@pytest.mark.parametrize("case", list(dc.DCONV_FWD), ids=_ID)
def test_dconv_forward_wide_channel_tiles(case):
    """The 64- and 32-channel tiles against the float64 restatement; the split is over Cout only and every workgroup
    runs the whole k-ordered chain, so an image of the batch has the bits of the same image run alone (which gets the
    16-channel tile), and the 2-channel offset form has the bits of the 18-channel form."""
    from acfm_video_3d_reconstruction_amd import ops
    N, Cin, Cout, H, W = case
    want_tile, grid_y = dc.DCONV_FWD[case]
    tile = _lib().acfm_deform_conv2d_channel_tile
    assert tile(N, H, W, Cout) == want_tile and (Cout + want_tile - 1) // want_tile == grid_y and tile(1, H, W, Cout) == 16
    d = _d()
    x, o18, o2, w, b = make_inputs(*dc.dconv_case6(case))
    r18, r2 = dc.dconv_refs(case)
    tx, t18, t2, tw = (torch.tensor(a, device=d) for a in (x, o18, o2, w))
    t2as18 = tile9(t2).contiguous()
    with torch.no_grad():
        for bias in (None, b):
            tb = None if bias is None else torch.tensor(bias, device=d)
            add = 0.0 if bias is None else bias.astype(np.float64)[None, :, None, None]
            got18 = ops.deform_conv2d(tx, t18, tw, tb)
            got2 = ops.deform_conv2d(tx, t2, tw, tb, shared_offset=True)
            assert got18.shape == got2.shape == (N, Cout, H, W) and got18.dtype == torch.float32
            tag = "dconv %s tile %d bias %s" % (case, want_tile, bias is not None)
            _allclose(tag + " 18 channels", got18, r18 + add)
            _allclose(tag + " 2 channels", got2, r2 + add)
            assert torch.equal(got2, ops.deform_conv2d(tx, t2as18, tw, tb)), tag + ": shared form != 18-channel form"
            assert torch.equal(got18, ops.deform_conv2d(tx, t18, tw, tb)), tag + ": a second run"
            for n in range(N):
                s = slice(n, n + 1)
                assert torch.equal(got18[s], ops.deform_conv2d(tx[s], t18[s], tw, tb)), (tag, "18 channels, image", n)
                assert torch.equal(got2[s], ops.deform_conv2d(tx[s], t2[s], tw, tb, shared_offset=True)), \
                    (tag, "2 channels, image", n)


# ------------------------------------------------------------------------------ deformable convolution, weight gradient
@pytest.mark.parametrize("case", list(dc.DCONV_WGRAD), ids=_ID)
def test_dconv_weight_gradient_over_several_tiles_per_workgroup(case):
    """per = 2 pixel tiles per workgroup of k_dconv_bwd_weight (accumulation across tiles, the barrier at the top of
    the loop), parts that get no tile and store zeros, the 1024-part cap, and at 31 x 31 workgroups whose two tiles lie
    in two images.  All four gradients against float64 autograd at the project's bound, for both offset forms; the
    offset, weight and bias gradients repeat their bits."""
    N, Cin, Cout, H, W = case
    split = dc.wgrad_split(N, Cin, H, W, Cout)
    assert {k: split[k] for k in dc.DCONV_WGRAD[case]} == dc.DCONV_WGRAD[case] and split["per"] > 1
    assert _lib().acfm_deform_conv2d_backward_workspace_bytes(N, Cin, H, W, Cout) == 4 * split["parts"] * Cout * 9 * Cin
    d = _d()
    x, o18, o2, w, b = make_inputs(*dc.dconv_case6(case))
    go = draw_go((N, Cout, H, W))
    for off in (o18, o2):
        off = nudge(off, H, W)
        ref = dconv_ref_grads(x, off, w, b, go)
        _, g = _dconv_grads(x, off, w, b, go, d)
        _, again = _dconv_grads(x, off, w, b, go, d)
        tag = "wgrad %s (%d parts of %d tiles, %d empty, %d across images) %d channels" % (
            case, split["parts"], split["per"], split["empty"], split["crossing"], off.shape[1])
        for name, a, r in zip(("grad_input", "grad_offset", "grad_weight", "grad_bias"), g, ref):
            assert a.dtype == torch.float32
            _ratio(tag + " " + name, a, r)
        for i, name in ((1, "grad_offset"), (2, "grad_weight"), (3, "grad_bias")):     # no atomics in these
            assert torch.equal(g[i], again[i]), (tag, name)


# ------------------------------------------------------------------------------ correlation
def _corr(f1, f2, md, d):
    from acfm_video_3d_reconstruction_amd import ops
    with torch.no_grad():
        return ops.correlation(torch.tensor(f1, device=d), torch.tensor(f2, device=d), md)


@pytest.mark.parametrize("case", list(dc.CORR_NO_SPLIT), ids=_ID)
def test_correlation_non_atomic_with_three_chunks(case):
    """768 one-tile images: k_correlation_fwd<md, false> over three 8-channel chunks, the last with 3 channels, on a
    partial 16 x 16 tile.  Against the float64 oracle; the same bits twice; the images run singly (the channel split
    with float atomics) agree at the same tolerance; and on a poisoned, fenced output every element is written."""
    from acfm_video_3d_reconstruction_amd import ops
    N, C, H, W, md = case
    split = _lib().acfm_correlation_channel_split
    assert split(N, C, H, W) == 1 and split(1, C, H, W) > 1
    d = _d()
    f1, f2 = dc.corr_inputs(case)
    ref = O.correlation(f1, f2, md)
    out, again = _corr(f1, f2, md, d), _corr(f1, f2, md, d)
    assert out.shape == ref.shape == (N, (2 * md + 1) ** 2, H, W)
    _allclose("correlation %s, no split" % (case,), out, ref)
    assert torch.equal(out, again)
    t1, t2 = torch.tensor(f1, device=d), torch.tensor(f2, device=d)
    with torch.no_grad():
        singly = torch.cat([ops.correlation(t1[n:n + 1], t2[n:n + 1], md) for n in range(N)])
    _allclose("correlation %s, images run singly (split)" % (case,), singly, ref)
    _allclose("correlation %s, batch against images run singly" % (case,), out, singly.double().cpu().numpy())
    with guards.armed("A") as g:
        poisoned = _corr(f1, f2, md, d)
    g.check()
    assert not g.unwritten(), g.unwritten()
    assert guards.same_bits(poisoned, out)


@pytest.mark.parametrize("case", list(dc.CORR_SPLIT), ids=_ID)
def test_correlation_atomic_at_displacement_one(case):
    N, C, H, W, md = case
    assert _lib().acfm_correlation_channel_split(N, C, H, W) == dc.CORR_SPLIT[case] > 1 and md == 1
    f1, f2 = dc.corr_inputs(case)
    out = _corr(f1, f2, md, _d())
    _allclose("correlation %s, split %d" % (case, dc.CORR_SPLIT[case]), out, O.correlation(f1, f2, md))


def test_correlation_layer_forward_and_backward_without_split():
    """The md = 4 case through correlation.Correlation under trainable(): the forward is the no-grad forward bit for
    bit (nothing is atomic here), both gradients against float64 autograd and the same bits twice."""
    case = next(c for c in dc.CORR_NO_SPLIT if c[4] == 4)
    N, C, H, W, md = case
    d = _d()
    f1, f2 = dc.corr_inputs(case)
    go = draw_go((N, (2 * md + 1) ** 2, H, W))
    ref = corr_ref_grads(f1, f2, md, go)
    out, g1, g2 = _corr_grads(f1, f2, md, go, d)
    out_b, b1, b2 = _corr_grads(f1, f2, md, go, d)
    _allclose("Correlation %s forward under trainable()" % (case,), out, O.correlation(f1, f2, md))
    assert torch.equal(out, _corr(f1, f2, md, d)) and torch.equal(out, out_b)
    _ratio("Correlation %s grad_f1" % (case,), g1, ref[0])
    _ratio("Correlation %s grad_f2" % (case,), g2, ref[1])
    assert torch.equal(g1, b1) and torch.equal(g2, b2)


# ------------------------------------------------------------------------------ LPIPS layer
def _lpips_data():
    """One draw at the wide shape; the narrow shape is its first 180 rows, so that both sides of the threshold see
    nearly the same data."""
    N, Nr, C, h, w = dc.LPIPS_WIDE
    g = torch.Generator().manual_seed(sum(dc.LPIPS_WIDE))
    return (L.features((N, C, h, w), g), L.features((Nr, C, h, w), g), torch.rand(C, generator=g),
            torch.randn(N, h, w, generator=g))


def _lpips_cut(shape):
    a, b, lin, gd = _lpips_data()
    h = shape[3]
    assert shape[:3] == dc.LPIPS_WIDE[:3] and shape[4] == dc.LPIPS_WIDE[4] and h <= dc.LPIPS_WIDE[3]
    return a[:, :, :h].contiguous(), b[:, :, :h].contiguous(), lin, gd[:, :h].contiguous()


@pytest.mark.parametrize("with_lin", [False, True], ids=["unit", "lin"])
@pytest.mark.parametrize("shape", list(dc.LPIPS), ids=_ID)
def test_lpips_layer_on_both_sides_of_the_wave_threshold(shape, with_lin):
    from acfm_video_3d_reconstruction_amd import ops
    N, Nr, C, h, w = shape
    assert dc.lpips_waves(N, h, w) == dc.LPIPS[shape]
    a, b, lin, gd = _lpips_cut(shape)
    dev = _d()
    lw = lin.to(dev) if with_lin else None
    lit = {}
    for dt in (torch.float64, torch.float32):
        x = a.to(dev, dt).requires_grad_(True)
        dd = L.lit_layer(x, b.to(dev, dt).repeat(N // Nr, 1, 1, 1), lw)[:, 0]
        lit[dt] = (dd.detach(),) + torch.autograd.grad(dd, [x], gd.to(dev, dt))
    x = a.to(dev).requires_grad_(True)
    dist = ops.lpips_layer(x, b.to(dev), lw)
    ga, = torch.autograd.grad(dist, [x], gd.to(dev))
    tag = "layer %s (%d waves)%s" % (shape, dc.LPIPS[shape], " lin" if with_lin else "")
    L.check(tag, dist, lit[torch.float32][0], lit[torch.float64][0])
    L.check(tag + " grad a", ga, lit[torch.float32][1], lit[torch.float64][1])


@pytest.mark.parametrize("with_lin", [False, True], ids=["unit", "lin"])
def test_lpips_wide_layer_with_a_zero_norm_pixel(with_lin):
    """One all-zero a pixel in the four-wave case (in the tile that holds the boundary between images 1 and 2): u = 0
    there, the gradient is finite and is q_c / (n_a + eps) - a_c (sum_k q_k a_k) / (n_a (n_a + eps)^2), q_c = 2 w_c
    (u_c - v_c) g, with the second term 0 where n_a = 0 -- the formula of test_gpu_lpips.test_layer_zero_norm_pixels
    with the channel weights added."""
    from acfm_video_3d_reconstruction_amd import ops
    shape = dc.LPIPS_WIDE
    N, Nr, C, h, w = shape
    a, b, lin, gd = _lpips_cut(shape)
    a = a.clone()
    a[2, :, 0, 3] = 0
    assert (2 * h * w + 3) // dc.LP_TILE == (2 * h * w - 1) // dc.LP_TILE     # the tile of the last pixel of image 1
    eps = 1e-10
    dev = _d()

    def formula(a, b, gd, lw):          # the stated definition and gradient, on one dtype
        b = b.repeat(N // Nr, 1, 1, 1)
        wc = 1.0 if lw is None else lw.to(a).reshape(1, -1, 1, 1)
        na, nb = (a * a).sum(1, keepdim=True).sqrt(), (b * b).sum(1, keepdim=True).sqrt()
        u, v = a / (na + eps), b / (nb + eps)
        dist = (wc * (u - v) ** 2).sum(1)
        q = 2 * wc * (u - v) * gd[:, None]
        second = a * (q * a).sum(1, keepdim=True) / torch.where(na > 0, na * (na + eps) ** 2, torch.ones_like(na))
        return dist, q / (na + eps) - torch.where(na > 0, second, torch.zeros_like(second))
    lw = lin.to(dev) if with_lin else None
    d64, g64 = formula(a.to(dev).double(), b.to(dev).double(), gd.to(dev).double(), lw)
    d32, g32 = formula(a.to(dev), b.to(dev), gd.to(dev), lw)
    x = a.to(dev).requires_grad_(True)
    dist = ops.lpips_layer(x, b.to(dev), lw)
    ga, = torch.autograd.grad(dist, x, gd.to(dev))
    assert bool(torch.isfinite(ga).all()) and bool(torch.isfinite(dist).all())
    tag = "wide layer, zero-norm pixel%s" % (" lin" if with_lin else "")
    L.check(tag + " forward", dist, d32, d64)
    # at the planted pixel u = 0, so d = sum_c w_c v_c^2 and the gradient is -2 w_c v_c g / eps: 1e9 and more, which
    # would set the bar of a comparison of the whole tensor; the pixel and the rest are held to the yardstick apart
    L.check(tag + " gradient at the pixel", ga[2, :, 0, 3], g32[2, :, 0, 3], g64[2, :, 0, 3])
    assert float(g64[2, :, 0, 3].abs().max()) > 1e8
    rest = torch.ones_like(ga)
    rest[2, :, 0, 3] = 0
    L.check(tag + " gradient everywhere else", ga * rest, g32 * rest, g64 * rest.double())


# ------------------------------------------------------------------------------ flat shading, deterministic mode
def test_one_face_in_every_slot_flat():
    """test_gpu_lit_shading.test_one_face_in_every_slot with mode="flat" and face normals: N = 1, 16 x 16, K = 8, all
    2048 slots on one face.  Default mode (k_phong_bwd<true, false>) and deterministic mode (<true, true>) against the
    float64 restatement at that file's bars; deterministic mode gives the same bits twice."""
    from acfm_video_3d_reconstruction_amd import _lib, ops
    d = _d()
    H, K = 16, 8
    verts, faces = _sphere(1, 12)
    p2f, zbuf, bary, dists, g = R.fragments(1, H, H, K, faces.shape[0], 13)
    lc, ref_light = _light(1, True, 10, False, d)
    # the face that faces the point light most squarely: lit, so that the position and the normal carry a gradient
    c, _ = ref_light.at(2)
    centre, (_, fn64) = verts.double()[faces].mean(1), R.normals(verts.double(), faces)
    lit = int(((fn64 * R.normalize(c["vec"] - centre)).sum(-1)).argmax())
    p2f = torch.full_like(p2f, lit)
    texels, G = torch.rand(1, H, H, K, 3, generator=g), torch.randn(1, H, H, K, 3, generator=g)
    table = ops.incidence_table(faces.to(d), verts.shape[0])

    def run():
        v, t = _leaf(verts, d), _leaf(texels, d)
        _, fn = ops.vertex_normals(v, faces.to(d), table)
        col = ops.phong_shade((p2f.to(d), zbuf.to(d), bary.to(d), dists.to(d)), v, faces.to(d), fn, t, lc, table,
                              mode="flat")
        return (col.detach(),) + torch.autograd.grad((col * G.to(d)).sum(), (t, v))

    rv, rt = _leaf(verts), _leaf(texels)
    ref = R.shade("flat", rv, faces, p2f, bary.double(), rt, ref_light)
    rgrads = torch.autograd.grad((ref * G.double()).sum(), (rt, rv))
    assert float(rgrads[1].abs().max()) > 1e-2                  # (a face in the dark would have no vertex gradient)
    got = run()
    R.close(got[0], ref, floor=0.0, what="one face, flat, colours")
    for gr, rr, name in zip(got[1:], rgrads, ("texels", "verts")):
        R.close(gr, rr, floor=1e-6, what="one face, flat, default mode, grad " + name)
    with _lib.raster_tuning(deterministic=True):
        x, y = run(), run()
    assert torch.equal(x[0], got[0])
    for a, b, rr, name in zip(x[1:], y[1:], rgrads, ("texels", "verts")):
        assert torch.equal(a, b), name
        R.close(a, rr, floor=1e-6, what="one face, flat, deterministic mode, grad " + name)


@pytest.mark.parametrize("point", [False, True], ids=["directional", "point"])
def test_flat_shade_deterministic_vs_float64(point):
    """(2, 9, 9), K = 8, flat, under raster_tuning(deterministic=True): per-mesh constants with shininess (10, 64), and
    shininess 0 as a number."""
    from acfm_video_3d_reconstruction_amd import _lib
    d = _d()
    for shin, per_mesh in ((torch.tensor([10.0, 64.0]), True), (0, False)):
        with _lib.raster_tuning(deterministic=True):
            col, grads, ref, rgrads = _shade_case((2, 9, 9), 8, "flat", point, shin, per_mesh, d)
        _check_shade(col, grads, ref, rgrads, shin, "(2, 9, 9) K8 flat deterministic point=%d s=%s" % (point, shin))


@pytest.mark.parametrize("mode", ["phong", "flat"])
def test_shininess_zero(mode):
    """relu(v.r)^0 is 1 wherever n.l > 0 -- also where v.r <= 0 -- and passes no gradient: the s == 0 branch of
    light_eval_bwd, in the default mode, as a number and per mesh (0 and 10)."""
    d = _d()
    for shin, per_mesh in ((0, False), (torch.tensor([0.0, 10.0]), True)):
        col, grads, ref, rgrads = _shade_case((2, 9, 9), 8, mode, True, shin, per_mesh, d)
        _check_shade(col, grads, ref, rgrads, shin, "(2, 9, 9) K8 %s s=%s" % (mode, shin))


# ------------------------------------------------------------------------------ atlas blend, the remaining K
ATLAS_K = sorted(set(FRAGMENT_K) - {c[1] for c in ATLAS_CASES})


@pytest.mark.parametrize("deterministic", [False, True], ids=["atomics", "deterministic"])
@pytest.mark.parametrize("K", ATLAS_K)
def test_atlas_blend_at_the_remaining_K(K, deterministic):
    """test_gpu_shader_fragments.test_atlas_texels, unchanged, at the K its cases leave out (R = 3, three crowded
    faces, an ambient [N,3], 1122 pixels), with float atomics and with the integer sums of deterministic mode."""
    from acfm_video_3d_reconstruction_amd import _lib
    assert ATLAS_K == [2, 8, 20, 32]
    if deterministic:
        with _lib.raster_tuning(deterministic=True):
            _atlas_texels(3, K, (2, 33, 17), True, 3)
    else:
        _atlas_texels(3, K, (2, 33, 17), True, 3)
