"""GPU: the remaining units on hostile, fenced memory (tests/guards.py run_case): the shaders through their public
operators (csrc/acfm_shade.hip, acfm_texuv.hip), the perceptual loss (acfm_lpips.hip), the texture head
(acfm_uvatlas.hip), geodesic handles (acfm_geodesic.hip) and the mask preparation (acfm_prep.hip).

Bits throughout: the scattering shader backwards run in the fixed-point mode (_lib.raster_tuning(deterministic=True),
whose 16 bytes of workspace per element are poisoned here), everything else is a gather or a fixed-order sum."""
import pytest
import torch

import guards
import handles_meshes as HM
import lpips_literal as L
from test_gpu_lpips import LAYER_SHAPES, _gen, _mask

pytestmark = pytest.mark.gpu
_report = guards.module_report(__name__)


def _d():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _leaf(t, d, grad=True):
    return t.clone().to(d).requires_grad_(grad)


# ------------------------------------------------------------------------------------------------ shading
def _fragments(N, H, W, K, Fm, seed):
    """Hand-built fragments: packed ids in [-1, N Fm) of the pixel's own mesh, barycentrics inside the face."""
    g = torch.Generator().manual_seed(seed)
    p2f = torch.randint(-1, Fm, (N, H, W, K), generator=g)
    p2f = torch.where(p2f >= 0, p2f + Fm * torch.arange(N).reshape(N, 1, 1, 1), p2f)
    bary = torch.rand(N, H, W, K, 3, generator=g) + 0.05
    bary = bary / bary.sum(-1, keepdim=True)
    zbuf = torch.where(p2f >= 0, 1.0 + torch.rand(N, H, W, K, generator=g), torch.tensor(-1.0))
    dists = torch.where(p2f >= 0, 1e-4 * torch.randn(N, H, W, K, generator=g), torch.tensor(-1.0))
    return p2f, zbuf, bary, dists, g


SHADE_SHAPES = [(1, 1, 1), (1, 5, 13)]        # P = 1 and P = 65: one lane, and one pixel past a wave


@pytest.mark.parametrize("shape", SHADE_SHAPES, ids=str)
def test_interpolate_face_attributes(shape):
    from acfm_video_3d_reconstruction_amd import _lib, ops
    d = _d()
    N, H, W = shape
    K, Fm, D = 2, 7, 3
    p2f, _, bary, _, g = _fragments(N, H, W, K, Fm, 1)
    attrs = torch.randn(N * Fm, 3, D, generator=g)
    G = torch.randn(N, H, W, K, D, generator=g)

    def fn(inp):
        b, a = inp(_leaf(bary, d)), inp(_leaf(attrs, d))
        with _lib.raster_tuning(deterministic=True):
            out = ops.interpolate_face_attributes(p2f.to(d), b, a)
            gb, ga = torch.autograd.grad(out, (b, a), inp(G.to(d)))
        return dict(out=out, gb=gb, ga=ga)
    guards.run_case(fn)


@pytest.mark.parametrize("shape", SHADE_SHAPES, ids=str)
def test_atlas_softmax_blend(shape):
    from acfm_video_3d_reconstruction_amd import _lib, ops
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.renderer import BlendParams
    d = _d()
    N, H, W = shape
    K, Fm, R = 2, 7, 3
    p2f, zbuf, bary, dists, g = _fragments(N, H, W, K, Fm, 2)
    atlas = torch.rand(N, Fm, R, R, 3, generator=g)
    G = torch.randn(N, H, W, 4, generator=g)
    bp = BlendParams(1e-4, 1e-2, (0.2, 0.5, 0.9))

    def fn(inp):
        a, z, dd = inp(_leaf(atlas, d)), inp(_leaf(zbuf, d)), inp(_leaf(dists, d))
        with _lib.raster_tuning(deterministic=True):
            out = ops.atlas_softmax_blend(a, (p2f.to(d), z, inp(bary.to(d)), dd), bp)
            ga, gz, gd = torch.autograd.grad(out, (a, z, dd), inp(G.to(d)))
        return dict(out=out, ga=ga, gz=gz, gd=gd)
    guards.run_case(fn)


@pytest.mark.parametrize("shape", SHADE_SHAPES, ids=str)
def test_sigmoid_and_softmax_blend(shape):
    """sigmoid_alpha_blend and the dense softmax_rgb_blend through the public operators (their kernels' outputs are
    fenced on the raw C ABI by test_gpu_shader_fragments.py; here the operators' own allocations are)."""
    from acfm_video_3d_reconstruction_amd import _lib, ops
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.renderer import BlendParams
    d = _d()
    N, H, W = shape
    K, Fm = 2, 7
    p2f, zbuf, bary, dists, g = _fragments(N, H, W, K, Fm, 4)
    colors = torch.rand(N, H, W, K, 3, generator=g)
    G = torch.randn(N, H, W, 4, generator=g)
    bp = BlendParams(1e-4, 1e-2, (0.2, 0.5, 0.9))

    def fn(inp):
        c, z, dd = inp(_leaf(colors, d)), inp(_leaf(zbuf, d)), inp(_leaf(dists, d))
        frags = (p2f.to(d), z, inp(bary.to(d)), dd)
        with _lib.raster_tuning(deterministic=True):
            sig = ops.sigmoid_alpha_blend(c, frags, bp)
            sc, sd = torch.autograd.grad(sig, (c, dd), inp(G.to(d)))
            sil = ops.sigmoid_alpha_blend(None, frags, bp)
            sd0, = torch.autograd.grad(sil, dd, inp(G.to(d)))
            soft = ops.softmax_rgb_blend(c, frags, bp)
            fc, fz, fd = torch.autograd.grad(soft, (c, z, dd), inp(G.to(d)))
        return dict(sig=sig, sc=sc, sd=sd, sil=sil, sd0=sd0, soft=soft, fc=fc, fz=fz, fd=fd)
    guards.run_case(fn)


@pytest.mark.parametrize("padding_mode", ["border", "zeros"])
@pytest.mark.parametrize("shape", SHADE_SHAPES, ids=str)
def test_uv_texels(shape, padding_mode):
    from acfm_video_3d_reconstruction_amd import _lib, ops
    d = _d()
    N, H, W = shape
    K, Fm, Hm, Wm = 2, 7, 5, 7
    p2f, _, bary, _, g = _fragments(N, H, W, K, Fm, 3)
    fv = torch.rand(N * Fm, 3, 2, generator=g) * 1.4 - 0.2          # [-0.2, 1.2]: taps fall outside the map
    maps = torch.rand(N, Hm, Wm, 3, generator=g)
    G = torch.randn(N, H, W, K, 3, generator=g)

    def fn(inp):
        b, f, m = inp(_leaf(bary, d)), inp(_leaf(fv, d)), inp(_leaf(maps, d))
        with _lib.raster_tuning(deterministic=True):
            out = ops.uv_texels(p2f.to(d), b, f, m, align_corners=True, padding_mode=padding_mode)
            gb, gf, gm = torch.autograd.grad(out, (b, f, m), inp(G.to(d)))
        return dict(out=out, gb=gb, gf=gf, gm=gm)
    guards.run_case(fn)


# ------------------------------------------------------------------------------------------------ perceptual loss
@pytest.mark.parametrize("N,Nr,H,W", [(1, 1, 5, 7), (4, 2, 5, 7)])
def test_lpips_input(N, Nr, H, W):
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    g = _gen(3)
    img = torch.rand(N, 3, H, W, generator=g)
    mask = _mask(Nr, H, W, g)
    mask[0, -1] = 0.5
    gy = torch.randn(N, 3, H, W, generator=g)

    def fn(inp):
        x = inp(_leaf(img, d))
        y = ops.lpips_input(x, inp(mask.to(d)))
        gx, = torch.autograd.grad(y, x, inp(gy.to(d)))
        return dict(y=y, gx=gx)
    guards.run_case(fn)


def test_lpips_layers_mask_weights_masked_mean():
    """Two layers side by side (the smallest LAYER_SHAPES entry, 5 channels on 4 x 4, and 67 channels on 9 x 5) with
    and without channel weights, their mask weights and the masked mean, with the backward through all of it."""
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    small = min(LAYER_SHAPES, key=lambda s: s[2] * s[3] * s[4] if s[3] > 1 else 1 << 30)
    assert small == (2, 2, 5, 4, 4)
    g = _gen(7)
    N, Nr, H, W = 2, 2, 17, 19
    shapes = [(5, 4, 4), (67, 9, 5)]
    fas = [L.features((N, C, h, w), g) for C, h, w in shapes]
    fbs = [L.features((Nr, C, h, w), g) for C, h, w in shapes]
    lins = [torch.rand(shapes[0][0], generator=g), None]
    mask = _mask(Nr, H, W, g)
    gl = torch.randn(N, generator=g)

    def fn(inp):
        a, b = [inp(_leaf(t, d)) for t in fas], [inp(_leaf(t, d)) for t in fbs]
        dmap = ops.lpips_layers(a, b, [lins[0].to(d), None])
        M = ops.lpips_mask_weights(inp(mask.to(d)), [(h, w) for _, h, w in shapes])
        loss = ops.lpips_masked_mean(dmap, M)
        grads = torch.autograd.grad(loss, a + b, inp(gl.to(d)))
        return dict(d=dmap, M=M, loss=loss, **{"g%d" % i: t for i, t in enumerate(grads)})
    guards.run_case(fn)


# ------------------------------------------------------------------------------------------------ texture head
@pytest.mark.parametrize("S", [5, 0])
def test_uv_atlas(S):
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    sampler = torch.rand(5, 3, 3, 2, generator=torch.Generator().manual_seed(4)) * 2 - 1
    uv = torch.randn(3, 3, 5, 7, generator=torch.Generator().manual_seed(5))
    G = torch.randn(3, 5 + S, 3, 3, 3, generator=torch.Generator().manual_seed(6))

    def fn(inp):
        table = ops.uv_atlas_table(inp(sampler.to(d)), 5, 7)
        x = inp(_leaf(uv, d))
        atlas = ops.uv_atlas(x, table, S)
        gx, = torch.autograd.grad(atlas, x, inp(G.to(d)))
        return dict(atlas=atlas, gx=gx, start=table.pix_start, taps=table.pix_taps)
    guards.run_case(fn)


# ------------------------------------------------------------------------------------------------ geodesic handles
@pytest.mark.parametrize("memory", ["lds", "device"])
def test_geodesic_distances(memory):
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    v, f = min((HM.square(), HM.l_shape()), key=lambda m: m[0].shape[0])
    verts = torch.tensor(v, dtype=torch.float32)
    faces = torch.tensor(f).to(d)

    def fn(inp):
        kw = dict(max_workgroups=3) if memory == "device" else {}
        return dict(D=ops.geodesic_distances(inp(verts.to(d)), faces, steiner=3, memory=memory, **kw),
                    some=ops.geodesic_distances(inp(verts.to(d))[None], faces, steiner=3, sources=[4, 0, 4], memory=memory, **kw))
    plain, _ = guards.run_case(fn)
    assert bool(torch.isfinite(plain["D"]).all()) and float(plain["D"].diagonal().abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ mask preparation
def test_mask_preparation():
    from acfm_video_3d_reconstruction_amd import image_utils as IU
    d = _d()
    H, W = 17, 19
    g = torch.Generator().manual_seed(8)
    masks = (torch.rand(3, H, W, generator=g) > 0.6).float()
    masks[1] = 0
    masks[1, 4:7, 5:8] = 1                                       # one 3 x 3 blob: a short boundary list
    masks[2] = 0                                                 # no boundary at all: count 0, every row padding

    def fn(inp):
        m = inp(masks.to(d))
        bd, counts = IU.compute_boundaries(m, cap=40, return_counts=True)
        grown = IU.compute_boundaries(m[:2])
        return dict(dt=IU.compute_dt(m), dt_raw=IU.compute_dt(m[0], norm=False), barrier=IU.compute_dt_barrier(m),
                    bd=bd, counts=counts, grown=grown)
    plain, _ = guards.run_case(fn)
    c = plain["counts"].tolist()
    assert c[2] == 0 and 0 < c[1] < 40 < c[0]                    # a list below the cap, one above it, an empty one
