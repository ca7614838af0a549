"""The shader kernels (acfm_shade.hip) on hand-built fragments: ops.sigmoid_alpha_blend / softmax_rgb_blend /
atlas_softmax_blend / interpolate_face_attributes fed with a plain (pix_to_face, zbuf, bary_coords, dists) tuple made
in numpy, no rasteriser involved, against the float64 restatements of tests/test_gpu_shaders.py.  A shader takes
fragments from any rasteriser or user code, so this is its contract: pixel counts that are no multiple of the wave,
H != W, every K of ops.FRAGMENT_K, holes in front of filled slots, ids below -1 and past F_packed, garbage in empty
slots, saturated sigmoids, every z_max / delta branch of the softmax blend and every edge of the atlas texel choice.

Bars (those of tests/test_gpu_shaders.py, through its _img / _close): images 1e-6; gradients 1e-4 of the reference's
scale plus the floor, and 1e-5 relative L2.  This file blends with znear = 0.5, zfar = 2.0 (both arguments of the
ops): at gamma = 1e-4 float32 cannot resolve z_inv of a few gamma next to zfar = 100.

The first two tests need no GPU: they pin the builder, so that no GPU test below passes on an empty population.
(That K outside ops.FRAGMENT_K and planes of mismatched shapes are refused is pinned by tests/test_shim_shaders.py.)"""
import ctypes
import functools
from collections import namedtuple

import numpy as np
import pytest
import torch

from test_gpu_shaders import (EPS, _close, _dev, _img, _leaf, _ref_alpha, _ref_interp, _ref_softmax,  # noqa: F401
                              _texel_index)

gpu = pytest.mark.gpu

SIGMA = 1e-4
ZNEAR, ZFAR = 0.5, 2.0
BG = (0.2, 0.5, 0.9)
GAMMAS = (1e-4, 1e-2)
FRAGMENT_K = (1, 2, 4, 8, 10, 20, 32)   # test_builder... asserts that this is ops.FRAGMENT_K
NEAR, FAR, BEYOND, TIGHT = 0, 1, 2, 3
REGIMES = ("near", "far", "beyond", "tight")
RANDOM, CORNER, GRID, UNCLIPPED, DIAGONAL = 0, 1, 3, 5, 7   # bary blocks: (p // 4) % 8, even values are RANDOM
GARBAGE = 3e20

# [N,H,W]: one pixel; P = 63; P = 65; H W = 63 (every wave spans two meshes of an ambient [N,3]); P = 1122 = 17 waves
# + 34 pixels (P K no multiple of 256 for odd K) and its transpose; an exact multiple of 64 as the control
SHAPES = ((1, 1, 1), (1, 3, 21), (1, 5, 13), (3, 7, 9), (2, 33, 17), (2, 17, 33), (2, 16, 32))
# every K meets the partial-wave shapes P = 63, 65, 1122; every shape meets K = 32
BLEND_CASES = [(s, K) for s in ((1, 3, 21), (1, 5, 13), (2, 33, 17)) for K in FRAGMENT_K] + \
              [((1, 1, 1), K) for K in (1, 10, 32)] + [((3, 7, 9), K) for K in (2, 8, 32)] + \
              [((2, 17, 33), K) for K in (4, 20, 32)] + [((2, 16, 32), K) for K in (8, 32)]
GUARD_CASES = [(s, K) for s in ((1, 1, 1), (1, 5, 13), (2, 33, 17)) for K in FRAGMENT_K]
REGIME_CASES = [((2, 33, 17), K) for K in (2, 4, 10, 32)] + [((1, 3, 21), 8), ((3, 7, 9), 20)]
# (R, K, shape, ambient, F_packed): R = 1, odd R, K in {1, 4, 10}, partial waves, an ambient [N,3] over waves that
# span two meshes; F_packed = 3 crowds a face, F_packed = 40 leaves most texels unreferenced
ATLAS_CASES = [(1, 1, (1, 5, 13), False, 5), (2, 4, (3, 7, 9), True, 5), (3, 10, (2, 33, 17), True, 3),
               (7, 4, (2, 33, 17), False, 40), (16, 1, (2, 17, 33), True, 40), (3, 1, (1, 3, 21), False, 3),
               (7, 10, (1, 5, 13), True, 40)]
INTERP_CASES = [((1, 5, 13), K, D) for K in (1, 10, 32) for D in (1, 3, 5, 17)] + \
               [((2, 33, 17), 32, 17), ((2, 33, 17), 10, 3), ((2, 33, 17), 1, 5), ((1, 1, 1), 1, 1)]

Built = namedtuple("Built", "pix_to_face zbuf bary_coords dists regime block faint")


def _seed(shape, K):
    return 100 * SHAPES.index(tuple(shape)) + K


def build_fragments(N, H, W, K, gamma, seed, F_packed, R=4, over=0.0):
    """Fragments no rasteriser writes, as float32 / int64 CPU tensors [N,H,W,K(,3)], plus per pixel its depth regime
    [N,H,W], its barycentric block and the `faint` flag.  p is the flat pixel index.

    ids: uniform in [0, F_packed); 30 % of the slots empty, each slot on its own, so holes precede filled slots; a
    tenth of the empty ones hold -5 instead of -1; pixels with p % 13 == 5 have all K slots filled, those with
    p % 13 == 11 none.  over > 0 turns that share of the filled slots into ids >= F_packed (F_packed, F_packed + 7,
    2^31 - 1): filled for the dense blends, empty for the atlas blend and the interpolation.

    depth regime (p + seed) % 4, so every regime sits inside every wave (and the one pixel of a 1 x 1 image changes
    regime with the seed):
      near    zbuf in [1, 1.5]: z_inv >= 1/3, delta at its 1e-10 clamp for both gammas (with zfar = 2 the natural
              scene's [1, 5] would cross zfar; the part of it in front of zfar is kept)
      far     the pixel's largest z_inv is drawn in (2 gamma, 20 gamma) and given to one random slot, the others lie up
              to 4 gamma below it; zbuf = zfar - z_inv (zfar - znear) in float64, then rounded: delta above its clamp
      beyond  zbuf >= zfar in every slot (half of them within 3 gamma of zfar, a tenth exactly zfar): z_max < eps
      tight   zbuf = z0 + j gamma (zfar - znear), j in {0..3} with repeats: several slots carry weight; in 60 % of
              these pixels two random slots are set to j = 0, an exact tie for the maximum between a lower- and a
              higher-numbered slot.  A quarter of the tight pixels are `faint`: dists in [20, 25] sigma, so that the
              sum of the weights is of the size of delta's clamp and the z_max term of the gradient (delta / gamma
              times ...) is as large as the others; with weights near 1 it is 1e-10 of them and no float32 test
              could tell which slot received it.

    dists: 3 sigma randn; 10 % at +0.02 and 10 % at -0.02 (+-200 sigma: expf overflows, p is exactly 0 or 1).

    bary, in runs of four pixels ((p // 4) % 8): 1 the three corners; 3 grid lines (w0 = i / R with w1 free, w1 = j / R
    with w0 free, and the grid's vertices); 5 unclipped values in [-0.5, 1.5]; 7 the diagonal, w1 = 1 - w0 in
    float32 so that w0 + w1 == 1 exactly; even values random barycentrics.

    Empty slots (id < 0) of dists, zbuf and bary are then overwritten with garbage of magnitude 3e20 (mostly the sign
    that would count if it were read: dists -3e20 is p = 1, zbuf -3e20 a huge z_inv), not with -1: the kernels must
    mask by id, never by value.  The garbage is finite because the float64 reference masks by multiplication, as
    PyTorch3D itself does (prob * mask, z_inv * mask): NaN or inf there would poison the reference, not the kernel."""
    rng = np.random.default_rng([seed, N, H, W, K])
    P = N * H * W
    p = np.arange(P)
    regime = (p + seed) % 4
    block = (p // 4) % 8
    block = np.where(block % 2 == 0, RANDOM, block)
    faint = ((p // 4) % 4 == 2) & (regime == TIGHT)
    rng_z = ZFAR - ZNEAR

    ids = rng.integers(0, F_packed, (P, K))
    u = rng.random((P, K))
    ids[u < 0.30] = -1
    ids[u < 0.03] = -5
    full, none = p % 13 == 5, p % 13 == 11
    ids[full] = rng.integers(0, F_packed, (int(full.sum()), K))
    ids[none] = np.where(rng.random((int(none.sum()), K)) < 0.2, -5, -1)
    if over > 0:
        sel = (rng.random((P, K)) < over) & (ids >= 0) & ~full[:, None]
        ids[sel] = rng.choice([F_packed, F_packed + 7, 2 ** 31 - 1], int(sel.sum()))
    filled = ids >= 0

    z = rng.uniform(1.0, 1.5, (P, K))                                           # near
    zmax = rng.uniform(2 * gamma, 20 * gamma, P)                                # far
    zi = zmax[:, None] - rng.uniform(0.0, 4 * gamma, (P, K))
    top = np.argmax(np.where(filled, rng.random((P, K)), -1.0), axis=1)
    zi[p, top] = zmax
    z = np.where((regime == FAR)[:, None], ZFAR - zi * rng_z, z)
    e = np.where(rng.random((P, K)) < 0.5, rng.uniform(0.0, 3 * gamma * rng_z, (P, K)), rng.uniform(0.0, 1.0, (P, K)))
    e[rng.random((P, K)) < 0.1] = 0.0                                           # beyond
    z = np.where((regime == BEYOND)[:, None], ZFAR + e, z)
    j = rng.integers(0, 4, (P, K)).astype(np.float64)                           # tight
    a, b = np.argsort(np.where(filled, rng.random((P, K)), 2.0), axis=1)[:, :2].T if K >= 2 else (top, top)
    tie = rng.random(P) < 0.6
    j[p[tie], a[tie]] = 0.0
    j[p[tie], b[tie]] = 0.0
    z0 = rng.uniform(1.0, 1.4, P)
    z = np.where((regime == TIGHT)[:, None], z0[:, None] + j * gamma * rng_z, z)

    d = 3 * SIGMA * rng.standard_normal((P, K))
    u = rng.random((P, K))
    d[u < 0.1] = 0.02
    d[(u >= 0.1) & (u < 0.2)] = -0.02
    d = np.where(faint[:, None], SIGMA * rng.uniform(20.0, 25.0, (P, K)), d)

    f32 = np.float32
    w = rng.dirichlet((1.0, 1.0, 1.0), (P, K)).astype(f32)
    k = np.arange(K)
    corner = np.eye(3, dtype=f32)[(p[:, None] + k[None, :]) % 3]
    i = rng.integers(0, R + 1, (P, K))
    g0 = i.astype(f32) / f32(R)
    g1 = (rng.random((P, K)).astype(f32) * (f32(1) - g0)).astype(f32)
    jv = rng.integers(0, R + 1, (P, K))
    jv = np.minimum(jv, R - i)                                                   # a vertex of the grid, i + j <= R
    kind = rng.integers(0, 3, (P, K))
    gw0 = np.where(kind == 0, g0, np.where(kind == 1, g1, g0))
    gw1 = np.where(kind == 0, g1, np.where(kind == 1, g0, jv.astype(f32) / f32(R)))
    grid = np.stack([gw0, gw1, f32(1) - gw0 - gw1], -1).astype(f32)
    d0 = rng.random((P, K)).astype(f32)
    diag = np.stack([d0, f32(1) - d0, np.zeros_like(d0)], -1).astype(f32)
    u01 = rng.uniform(-0.5, 1.5, (P, K, 2)).astype(f32)
    uncl = np.concatenate([u01, (f32(1) - u01[..., :1] - u01[..., 1:])], -1).astype(f32)
    for tag, val in ((CORNER, corner), (GRID, grid), (UNCLIPPED, uncl), (DIAGONAL, diag)):
        w = np.where((block == tag)[:, None, None], val, w)

    empty = ids < 0
    flip = rng.random((P, K)) < 0.25
    d = np.where(empty, np.where(flip, GARBAGE, -GARBAGE), d)
    z = np.where(empty, np.where(flip, 7e20, -GARBAGE), z)
    w = np.where(empty[..., None], f32(GARBAGE), w)

    def t(x, *tail):
        return torch.from_numpy(np.ascontiguousarray(x)).reshape((N, H, W) + tail)
    return Built(t(ids.astype(np.int64), K), t(z.astype(f32), K), t(w.astype(f32), K, 3), t(d.astype(f32), K),
                 t(regime), t(block), t(faint))


def _mask_over(p2f, F_packed):
    """An id >= F_packed is empty for the reference, exactly as an id < 0 is."""
    return torch.where(p2f >= F_packed, torch.full_like(p2f, -1), p2f)


def _ref_softmax_const_zmax(p2f, dists, zbuf, colors, gamma):
    """_ref_softmax with z_max taken as a constant: the gradient without its z_max term."""
    mask = (p2f >= 0).double()
    prob, alpha = _ref_alpha(p2f, dists, SIGMA)
    z_inv = (ZFAR - zbuf) / (ZFAR - ZNEAR) * mask
    z_max = torch.max(z_inv, dim=-1).values[..., None].clamp(min=EPS).detach()
    w = prob * torch.exp((z_inv - z_max) / gamma)
    delta = torch.exp((EPS - z_max) / gamma).clamp(min=EPS)
    denom = w.sum(dim=-1)[..., None] + delta
    rgb = ((w[..., None] * colors).sum(dim=-2) + delta * torch.as_tensor(BG, dtype=torch.float64)) / denom
    return torch.cat([rgb, alpha[..., None]], dim=-1)


def _f32_softmax(p2f, dists, zbuf, colors, gamma):
    """The blend as the kernel states it, in float32 torch: z_inv and the arguments of the exponentials in float64,
    everything else (sigmoid, exponentials, sums, the division) in float32."""
    mask = p2f >= 0
    prob = torch.sigmoid(-dists / SIGMA) * mask
    alpha = 1.0 - torch.prod(1.0 - prob, dim=-1)
    z_inv = (ZFAR - zbuf.double()) / (ZFAR - ZNEAR) * mask
    z_max = torch.max(z_inv, dim=-1).values[..., None].clamp(min=EPS)
    w = prob * torch.exp(((z_inv - z_max) / gamma).float())
    delta = torch.exp(((EPS - z_max) / gamma).float()).clamp(min=EPS)
    denom = w.sum(dim=-1)[..., None] + delta
    rgb = ((w[..., None] * colors).sum(dim=-2) + delta * torch.tensor(BG)) / denom
    return torch.cat([rgb, alpha[..., None]], dim=-1)


def _z_stats(p2f, zbuf, gamma):
    """The reference's own z_inv, raw z_max (before its clamp), raw delta (before its clamp) and the tie mask."""
    mask = (p2f >= 0).double()
    z_inv = (ZFAR - zbuf.double()) / (ZFAR - ZNEAR) * mask
    z_raw = z_inv.max(dim=-1).values
    delta_raw = torch.exp((EPS - z_raw.clamp(min=EPS)) / gamma)
    at_max = (z_inv == z_raw[..., None]) & (p2f >= 0)
    return z_inv, z_raw, delta_raw, at_max


SoftCase = namedtuple("SoftCase", "b colors G ref g_dists g_zbuf g_colors g_zbuf_const")


@functools.lru_cache(maxsize=None)
def _soft_case(shape, K, gamma):
    """Dense softmax case of (shape, K, gamma): fragments, colours, the upstream gradient and the float64 reference
    image and gradients (with and without the z_max term), computed once and shared."""
    N, H, W = shape
    b = build_fragments(N, H, W, K, gamma, _seed(shape, K), 50)
    g = torch.Generator().manual_seed(_seed(shape, K))
    colors = torch.rand(N, H, W, K, 3, generator=g)
    G = torch.randn(N, H, W, 4, generator=g)
    rd, rz, rc = _leaf(b.dists), _leaf(b.zbuf), _leaf(colors)
    ref = _ref_softmax(b.pix_to_face, rd, rz, rc, SIGMA, gamma, BG, ZNEAR, ZFAR)
    gd, gz, gc = torch.autograd.grad(ref, [rd, rz, rc], G.double())
    (gzc,) = torch.autograd.grad(_ref_softmax_const_zmax(b.pix_to_face, rd, rz, rc, gamma), [rz], G.double())
    return SoftCase(b, colors, G, ref.detach(), gd, gz, gc, gzc)


SigCase = namedtuple("SigCase", "b colors G ref g_dists g_colors")


@functools.lru_cache(maxsize=None)
def _sig_case(shape, K, with_colors):
    b = _soft_case(shape, K, GAMMAS[0]).b
    N, H, W = shape
    g = torch.Generator().manual_seed(_seed(shape, K) + 1)
    colors = torch.rand(N, H, W, K, 3, generator=g) if with_colors else None
    G = torch.randn(N, H, W, 4, generator=g)
    rd = _leaf(b.dists)
    rc = _leaf(colors) if with_colors else None
    _, alpha = _ref_alpha(b.pix_to_face, rd, SIGMA)
    rgb = rc[..., 0, :] if with_colors else torch.ones(N, H, W, 3, dtype=torch.float64)
    ref = torch.cat([rgb, alpha[..., None]], -1)
    grads = torch.autograd.grad(ref, [rd, rc] if with_colors else [rd], G.double())
    return SigCase(b, colors, G, ref.detach(), grads[0], grads[1] if with_colors else None)


ONE_PIXEL_MARGIN = 8.0


@functools.lru_cache(maxsize=None)
def _floors(shape, K, gamma):
    """The floor of the gradient bars (1e-4 of scale + floor), per gradient, for the blends of _soft_case (gamma) or
    _sig_case (gamma None): the suite's 1e-9, except on the one-pixel image.  There the scale of a gradient is one
    pixel's own gradient, which can be as small as it likes (1e-5 where a slot has p next to 1), while rounding p to
    float32 moves the gradient to dists by up to 2^-24 / sigma = 6e-4 of the upstream gradient whatever the scale
    is: rounding, not a defect.  So the one-pixel cases take as floor the error of the float32 CPU restatement
    (_f32_softmax, never the kernel's output) on the same pixel times ONE_PIXEL_MARGIN = 8 (the kernel's sigmoid,
    1 / (1 + expf(x)), rounds 1 - p differently from torch.sigmoid: up to a few ulp of 1), and never less than 1e-9."""
    out = dict(d=1e-9, z=1e-9, c=1e-9)
    if int(np.prod(shape)) != 1:
        return out
    if gamma is None:
        c = _sig_case(shape, K, True)
        d, col = (t.clone().requires_grad_(True) for t in (c.b.dists, c.colors))
        prob = torch.sigmoid(-d / SIGMA) * (c.b.pix_to_face >= 0)
        img = torch.cat([col[..., 0, :], (1.0 - torch.prod(1.0 - prob, dim=-1))[..., None]], -1)
        got = dict(zip("dc", torch.autograd.grad(img, [d, col], c.G)))
        want = dict(d=c.g_dists, c=c.g_colors)
    else:
        c = _soft_case(shape, K, gamma)
        d, z, col = (t.clone().requires_grad_(True) for t in (c.b.dists, c.b.zbuf, c.colors))
        img = _f32_softmax(c.b.pix_to_face, d, z, col, gamma)
        got = dict(zip("dzc", torch.autograd.grad(img, [d, z, col], c.G)))
        want = dict(d=c.g_dists, z=c.g_zbuf, c=c.g_colors)
    for k in got:
        out[k] = max(1e-9, ONE_PIXEL_MARGIN * float((got[k].double() - want[k]).abs().max()))
    return out


def _covered(p2f):
    return (p2f >= 0).any(dim=-1)


def _faint_ties(b, gamma, F_packed=None):
    """Faint tight pixels whose maximal z_inv is shared by two or more filled slots."""
    p2f = b.pix_to_face if F_packed is None else _mask_over(b.pix_to_face, F_packed)
    _, z_raw, _, at_max = _z_stats(p2f, b.zbuf, gamma)
    return b.faint & (at_max.sum(-1) >= 2) & (z_raw > EPS)


# ------------------------------------------------------------------------------ the builder (no GPU)
def test_builder_populates_every_regime_and_float32_meets_the_bars():
    """For every (shape, K, gamma) of the GPU tests: the float64 reference and its gradients are finite; of the covered
    pixels at least 10 % lie in each of the four regimes, counted by the reference's own numbers (far: delta above
    its clamp and z_max > eps; beyond: z_max <= eps; near and tight: delta at its clamp); for K >= 2 at least 5 % of
    the tight pixels tie exactly for the maximum (and some of those are faint); holes precede filled slots, ids of
    -5, full and empty pixels, +-200 sigma and garbage are all present; and the float32 restatement of the blend
    (_f32_softmax: what the kernel computes, in torch on the CPU) stays within the suite's bars of the float64
    reference.  (Population shares are asserted for P >= 63; a 1 x 1 image holds one pixel, whose regime moves with
    the seed.)  torch.max sends the gradient of a tie to the first maximal slot: pinned here, because the tie case
    relies on it."""
    from acfm_video_3d_reconstruction_amd import ops
    assert tuple(ops.FRAGMENT_K) == FRAGMENT_K
    x = torch.tensor([[1.0, 3.0, 3.0, 2.0]], dtype=torch.float64, requires_grad=True)
    x.max(dim=-1).values.sum().backward()
    assert x.grad.tolist() == [[0.0, 1.0, 0.0, 0.0]]

    cases = sorted(set(BLEND_CASES) | set(GUARD_CASES) | set(REGIME_CASES))
    assert {K for _, K in BLEND_CASES} == set(FRAGMENT_K) and {s for s, _ in BLEND_CASES} == set(SHAPES)
    assert all((s, 32) in BLEND_CASES for s in SHAPES)
    worst = dict(img=0.0, scale=0.0, rel=0.0)
    single = set()
    for shape, K in cases:
        for gamma in GAMMAS:
            c = _soft_case(shape, K, gamma)
            b = c.b
            P = b.regime.numel()
            for t in (c.ref, c.g_dists, c.g_zbuf, c.g_colors, c.g_zbuf_const):
                assert bool(torch.isfinite(t).all()), (shape, K, gamma)
            cov = _covered(b.pix_to_face)
            _, z_raw, delta_raw, at_max = _z_stats(b.pix_to_face, b.zbuf, gamma)
            by_ref = {FAR: (delta_raw > EPS) & (z_raw > EPS), BEYOND: z_raw <= EPS,
                      NEAR: delta_raw <= EPS, TIGHT: delta_raw <= EPS}
            for r, name in enumerate(REGIMES):
                m = (b.regime == r) & cov
                assert bool(by_ref[r][m].all()), (shape, K, gamma, name)
                if P >= 63:
                    assert int(m.sum()) >= 0.10 * int(cov.sum()), (shape, K, gamma, name)
                else:
                    single.add(int(b.regime.reshape(-1)[0]))
            if P >= 63:
                p2f = b.pix_to_face
                assert bool(((p2f[..., :-1] < 0) & (p2f[..., 1:] >= 0)).any()) or K == 1
                assert bool((p2f == -5).any()) and bool((p2f >= 0).all(-1).any()) and bool((p2f < 0).all(-1).any())
                assert bool(((b.dists == 0.02) & (p2f >= 0)).any()) and bool(((b.dists == -0.02) & (p2f >= 0)).any())
                empty = p2f < 0
                for t in (b.dists, b.zbuf, b.bary_coords[..., 0]):
                    assert bool((t[empty].abs() >= 1e20).all()) and bool(torch.isfinite(t).all())
                if K >= 2:
                    tight = (b.regime == TIGHT) & cov
                    ties = tight & (at_max.sum(-1) >= 2)
                    assert int(ties.sum()) >= 0.05 * int(tight.sum()), (shape, K, gamma)
                    if (shape, K) in REGIME_CASES:
                        assert int(_faint_ties(b, gamma).sum()) >= 1, (shape, K, gamma)
            # the float32 restatement against the float64 reference
            d, z, col = (t.clone().requires_grad_(True) for t in (b.dists, b.zbuf, c.colors))
            out = _f32_softmax(b.pix_to_face, d, z, col, gamma)
            assert out.dtype == torch.float32
            gd, gz, gc = torch.autograd.grad(out, [d, z, col], c.G)
            worst["img"] = max(worst["img"], float((out.detach().double() - c.ref).abs().max()))
            for got, ref in ((gd, c.g_dists), (gz, c.g_zbuf), (gc, c.g_colors)):
                scale = float(ref.abs().max())
                if scale > 0 and P >= 63:
                    worst["scale"] = max(worst["scale"], float((got.double() - ref).abs().max()) / scale)
                    worst["rel"] = max(worst["rel"], float((got.double() - ref).norm() / ref.norm()))
            tag = "float32 restatement %s K=%d gamma=%g" % (shape, K, gamma)
            fl = _floors(shape, K, gamma)      # 1e-9, but for the one-pixel image (there: this restatement's error x 8)
            _img(out, c.ref, what=tag + " image")
            _close(gd, c.g_dists, floor=fl["d"], what=tag + " grad dists")
            _close(gz, c.g_zbuf, floor=fl["z"], what=tag + " grad zbuf")
            _close(gc, c.g_colors, floor=fl["c"], what=tag + " grad colours")
    assert len(single) >= 2, "the one-pixel image must visit more than one regime over its cases"
    print("float32 restatement, worst over %d cases: image %.3g, gradient %.3g of scale, %.3g relative L2"
          % (2 * len(cases), worst["img"], worst["scale"], worst["rel"]))


def test_builder_barycentric_blocks_reach_the_texel_edges():
    """For every atlas case: the corner block holds all three corners; the diagonal block has w0 + w1 == 1 exactly in
    float32; the grid block has w R exactly on a grid line; the unclipped block goes below 0 and above 1; some ids
    are >= F_packed.  For R = 3 and F_packed = 3 the grid-line block alone references every texel of face 0 with
    x + y <= R - 1, and all fragments together all nine.  (A point on a grid line has one fractional part equal to
    zero, so it can never be mirrored: the texels above the diagonal are reached only by the mirror, which the
    random and unclipped blocks exercise.)"""
    for R, K, shape, _, Fp in ATLAS_CASES:
        b, p2f = _atlas_fragments(R, K, shape, Fp)
        valid = p2f >= 0
        w = b.bary_coords
        blk = b.block[..., None].expand_as(p2f)
        big = p2f.numel() > 1000          # the small cases hold a handful of slots per block
        corners = {(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)}
        c = {tuple(r) for r in w[(blk == CORNER) & valid].tolist()}
        assert c == corners if big or K > 1 else (len(c) > 0 and c <= corners)
        dg = w[(blk == DIAGONAL) & valid]
        assert len(dg) > 0 and bool(((dg[:, 0] + dg[:, 1]) == 1.0).all())
        gr = w[(blk == GRID) & valid]
        on_line = ((gr[:, 0] * R) == (gr[:, 0] * R).round()) | ((gr[:, 1] * R) == (gr[:, 1] * R).round())
        print("R=%d K=%d %s: %d grid-line slots, %.2f of them with w R an integer in float32"
              % (R, K, shape, len(gr), float(on_line.float().mean())))
        assert len(gr) > 0 and float(on_line.float().mean()) > 0.5
        un = w[(blk == UNCLIPPED) & valid]
        assert len(un) > 0
        if big:
            assert bool((b.pix_to_face >= Fp).any())
            assert float(un.min()) < -0.3 and float(un[:, :2].max()) > 1.3
        if R == 3 and Fp == 3 and big:
            ti = _texel_index(p2f, w, R)
            face0 = valid & (p2f == 0)
            assert set(ti[face0].tolist()) == set(range(9))
            lower = {y * R + x for x in range(R) for y in range(R) if x + y <= R - 1}
            assert lower <= set(ti[face0 & (blk == GRID)].tolist())


# ------------------------------------------------------------------------------ GPU helpers
PAD = 4096       # floats on either side of a guarded buffer: more than the 63 x 33 words a wave's rows hold
SENTINEL = -777.25


class _Guards:
    """Output buffers carved out of larger tensors filled with a sentinel: a kernel that writes one element before or
    past its output changes the sentinel (a torch.empty neighbour would hide it), and one that skips an element leaves
    the sentinel inside."""

    def __init__(self, dev):
        self.dev, self.bufs = dev, []

    def __call__(self, *shape):
        n = int(np.prod(shape))
        big = torch.full((n + 2 * PAD,), SENTINEL, dtype=torch.float32, device=self.dev)
        self.bufs.append((big, n, shape))
        return big[PAD:PAD + n].view(shape)

    def check(self, what):
        torch.cuda.synchronize()
        for big, n, shape in self.bufs:
            assert bool((big[:PAD] == SENTINEL).all()), "%s: a write before a %s output" % (what, shape)
            assert bool((big[PAD + n:] == SENTINEL).all()), "%s: a write past a %s output" % (what, shape)
            assert not bool((big[PAD:PAD + n] == SENTINEL).any()), "%s: a %s output not fully written" % (what, shape)


def _bp(gamma):
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.renderer import BlendParams
    return BlendParams(SIGMA, gamma, BG)


def _frag_tuple(b, dev, dists=None, zbuf=None, bary=None):
    return (b.pix_to_face.to(dev), zbuf if zbuf is not None else b.zbuf.to(dev),
            bary if bary is not None else b.bary_coords.to(dev), dists if dists is not None else b.dists.to(dev))


def _grads(out, inputs, G):
    return torch.autograd.grad(out, inputs, G, retain_graph=True)


# ------------------------------------------------------------------------------ blends: every K, partial waves
@gpu
@pytest.mark.parametrize("shape,K", BLEND_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_blends_every_K_and_partial_waves(shape, K):
    """sigmoid_alpha_blend (without and with colours) and the dense softmax_rgb_blend (gamma 1e-4 and 1e-2, a
    non-grey background) on built fragments: image and the gradients to dists, zbuf and colours against float64.

    Reaches: stage_rows / unstage_rows with P - p0 < 64 and the npix arithmetic of the contiguous grad_colors store
    (P = 1, 63, 65, 1122), H != W through ops._frag_planes, and the with_k instantiations K = 2, 4, 10, 32 (K = 32:
    pk[32], w[32], qk[32], double zi[32] per lane).  The fragments hold what a rasteriser never writes: empty slots
    in front of filled ones, pixels with all K slots filled, ids of -5, and +-3e20 instead of -1 in the empty slots
    of dists and zbuf.  Each backward is also run with only one input requiring a
    gradient, so the kernels run with g_dists, g_zbuf or g_colors NULL; those results must equal the joint ones bit
    for bit (no atomics on this path).  That nothing is written past P is checked by
    test_blends_write_nothing_outside_their_outputs, where the outputs are carved out of guard tensors."""
    from acfm_video_3d_reconstruction_amd import ops
    dev = _dev()
    N, H, W = shape
    for with_colors in (False, True):
        c = _sig_case(shape, K, with_colors)
        dists = c.b.dists.to(dev).requires_grad_(True)
        col = c.colors.to(dev).requires_grad_(True) if with_colors else None
        out = ops.sigmoid_alpha_blend(col, _frag_tuple(c.b, dev, dists=dists), _bp(1e-4))
        assert out.shape == (N, H, W, 4)
        tag = "sigmoid %s K=%d colours=%s" % (shape, K, with_colors)
        _img(out, c.ref, what=tag + " image")
        G = c.G.to(dev)
        got = _grads(out, [dists, col] if with_colors else [dists], G)
        fl = _floors(shape, K, None)
        _close(got[0], c.g_dists, floor=fl["d"], what=tag + " grad dists")
        if with_colors:
            _close(got[1], c.g_colors, floor=fl["c"], what=tag + " grad colours")
            for i in range(2):                             # g_colors NULL, then g_dists NULL
                d1 = dists.detach().requires_grad_(i == 0)
                c1 = col.detach().requires_grad_(i == 1)
                o1 = ops.sigmoid_alpha_blend(c1, _frag_tuple(c.b, dev, dists=d1), _bp(1e-4))
                (g1,) = _grads(o1, [d1 if i == 0 else c1], G)
                assert torch.equal(g1, got[i]), tag + " single gradient %d" % i
    for gamma in GAMMAS:
        c = _soft_case(shape, K, gamma)
        dists = c.b.dists.to(dev).requires_grad_(True)
        zbuf = c.b.zbuf.to(dev).requires_grad_(True)
        col = c.colors.to(dev).requires_grad_(True)
        out = ops.softmax_rgb_blend(col, _frag_tuple(c.b, dev, dists=dists, zbuf=zbuf), _bp(gamma), znear=ZNEAR,
                                    zfar=ZFAR)
        assert out.shape == (N, H, W, 4)
        tag = "softmax %s K=%d gamma=%g" % (shape, K, gamma)
        _img(out, c.ref, what=tag + " image")
        G = c.G.to(dev)
        got = _grads(out, [dists, zbuf, col], G)
        fl = _floors(shape, K, gamma)
        _close(got[0], c.g_dists, floor=fl["d"], what=tag + " grad dists")
        _close(got[1], c.g_zbuf, floor=fl["z"], what=tag + " grad zbuf")
        _close(got[2], c.g_colors, floor=fl["c"], what=tag + " grad colours")
        for i in range(3):                                 # one of g_dists / g_zbuf / g_colors, the other two NULL
            leaves = [t.detach().requires_grad_(i == j) for j, t in enumerate((dists, zbuf, col))]
            o1 = ops.softmax_rgb_blend(leaves[2], _frag_tuple(c.b, dev, dists=leaves[0], zbuf=leaves[1]), _bp(gamma),
                                       znear=ZNEAR, zfar=ZFAR)
            (g1,) = _grads(o1, [leaves[i]], G)
            assert torch.equal(g1, got[i]), tag + " single gradient %d" % i


@gpu
@pytest.mark.parametrize("shape,K", GUARD_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_blends_write_nothing_outside_their_outputs(shape, K):
    """The blends' entry points called with every output and gradient carved out of a sentinel-filled guard tensor
    (P = 1, 65 and 1122: the last wave is partial): the guards on both sides stay untouched, every element inside is
    written, and what is inside meets the float64 reference.  This is what catches unstage_rows or the grad_colors
    store running over a full wave's 64 rows where P - p0 < 64 remain."""
    from acfm_video_3d_reconstruction_amd import _lib, ops
    dev = _dev()
    N, H, W = shape
    P = N * H * W
    q = _lib.ptr
    c = _sig_case(shape, K, True)
    b = c.b
    p2f, ds = b.pix_to_face.to(dev).contiguous(), b.dists.to(dev).contiguous()
    cols = c.colors.to(dev).contiguous()
    g = c.G.to(dev).contiguous()
    guards = _Guards(dev)
    rgba, gd, gc = guards(N, H, W, 4), guards(N, H, W, K), guards(N, H, W, K, 3)
    _lib.call("acfm_sigmoid_alpha_blend", dev, q(p2f), q(ds), q(cols), P, K, SIGMA, q(rgba), None)
    _lib.call("acfm_sigmoid_alpha_blend_backward", dev, q(p2f), q(ds), q(g), P, K, SIGMA, q(gd), q(gc), None)
    tag = "guarded sigmoid %s K=%d" % (shape, K)
    guards.check(tag)
    _img(rgba, c.ref, what=tag + " image")
    fl = _floors(shape, K, None)
    _close(gd, c.g_dists, floor=fl["d"], what=tag + " grad dists")
    _close(gc, c.g_colors, floor=fl["c"], what=tag + " grad colours")
    for gamma in GAMMAS:
        c = _soft_case(shape, K, gamma)
        b = c.b                                            # (zbuf depends on gamma)
        p2f, ds, zb = b.pix_to_face.to(dev).contiguous(), b.dists.to(dev).contiguous(), b.zbuf.to(dev).contiguous()
        cols, g = c.colors.to(dev).contiguous(), c.G.to(dev).contiguous()
        bp = ops.blend_struct(_bp(gamma), ZNEAR, ZFAR)
        guards = _Guards(dev)
        rgba, gd, gz, gc = guards(N, H, W, 4), guards(N, H, W, K), guards(N, H, W, K), guards(N, H, W, K, 3)
        _lib.call("acfm_softmax_rgb_blend", dev, q(p2f), q(ds), q(zb), None, q(cols), None, 0, 0, None, P, K, H * W,
                  ctypes.byref(bp), q(rgba), None)
        _lib.call("acfm_softmax_rgb_blend_backward", dev, q(p2f), q(ds), q(zb), None, q(cols), None, 0, 0, None, P, K,
                  H * W, ctypes.byref(bp), q(g), q(gd), q(gz), q(gc), None, None, 0, None)
        tag = "guarded softmax %s K=%d gamma=%g" % (shape, K, gamma)
        guards.check(tag)
        _img(rgba, c.ref, what=tag + " image")
        fl = _floors(shape, K, gamma)
        _close(gd, c.g_dists, floor=fl["d"], what=tag + " grad dists")
        _close(gz, c.g_zbuf, floor=fl["z"], what=tag + " grad zbuf")
        _close(gc, c.g_colors, floor=fl["c"], what=tag + " grad colours")


# ------------------------------------------------------------------------------ softmax: the z_max / delta branches
@gpu
@pytest.mark.parametrize("shape,K", REGIME_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_softmax_depth_regimes(shape, K):
    """The gradient to zbuf of the dense softmax blend, regime by regime: each regime's pixels are compared on their
    own, with their own scale, so the large gradients of one regime cannot hide an error in another.

    near / tight  delta at its 1e-10 clamp: delta_live false, the gzmax term is taken
    far           delta above its clamp (z_max below about 23 gamma) with faces in the pixel: the kernel sets
                  gzmax = 0 because the two z_max paths cancel exactly; the float64 autograd walks both paths
    beyond        every filled zbuf >= zfar, z_max < eps: zmax_live false.  The clamped maximum passes no gradient:
                  the reference with z_max held constant gives the same gradient there, and the kernel meets it
    ties          in faint tight pixels (sum of weights of the size of delta, so that the gzmax term is as large as
                  the others) whose maximum is tied exactly, the gzmax share -- the gradient minus the gradient with
                  z_max held constant -- sits on the first tied slot only, as torch.max gives it, and the kernel's
                  share (its gradient minus the same constant-z_max reference) meets it
    The reference's (p2f >= 0) covers the ids of -5; gradients are exactly 0 in every empty slot."""
    from acfm_video_3d_reconstruction_amd import ops
    dev = _dev()
    for gamma in GAMMAS:
        c = _soft_case(shape, K, gamma)
        b = c.b
        zbuf = b.zbuf.to(dev).requires_grad_(True)
        out = ops.softmax_rgb_blend(c.colors.to(dev), _frag_tuple(b, dev, zbuf=zbuf), _bp(gamma), znear=ZNEAR,
                                    zfar=ZFAR)
        (gz,) = _grads(out, [zbuf], c.G.to(dev))
        gz = gz.double().cpu()
        assert bool(torch.isfinite(gz).all())
        assert bool((gz[b.pix_to_face < 0] == 0).all())
        cov = _covered(b.pix_to_face)
        tag = "softmax %s K=%d gamma=%g grad zbuf, " % (shape, K, gamma)
        for r, name in enumerate(REGIMES):
            m = (b.regime == r) & cov
            assert int(m.sum()) > 0
            _close(gz[m], c.g_zbuf[m], what=tag + name)
        m = (b.regime == BEYOND) & cov
        assert torch.equal(c.g_zbuf[m], c.g_zbuf_const[m])
        _close(gz[m], c.g_zbuf_const[m], what=tag + "beyond, z_max constant")
        if K >= 2:
            m = _faint_ties(b, gamma)
            assert int(m.sum()) >= 1
            _, _, _, at_max = _z_stats(b.pix_to_face, b.zbuf, gamma)
            first = at_max[m] & (at_max[m].long().cumsum(-1) == 1)
            share_ref = (c.g_zbuf - c.g_zbuf_const)[m]
            scale = float(share_ref.abs().max())
            assert scale > 1e-3 * float(c.g_zbuf[m].abs().max()), "the z_max share must not vanish in the gradient"
            assert float(share_ref[~first].abs().max()) <= 1e-12 * scale       # the reference: the first tied slot
            _close(gz[m] - c.g_zbuf_const[m], share_ref, what=tag + "z_max share of exact ties")


# ------------------------------------------------------------------------------ sigmoid: saturation and garbage
@gpu
@pytest.mark.parametrize("K", [1, 4, 32])
def test_sigmoid_saturation_and_garbage(K):
    """dists of +-200 sigma: expf overflows to inf or underflows to 0 and p must be exactly 0 or 1 -- with K = 1 the
    alpha channel is p itself; a pixel with a p = 1 slot has A == 1 and exactly zero gradient on all its dists; a
    pixel whose filled slots are all at +200 sigma has A == 0.  Outputs and gradients of both blends are finite
    everywhere and exactly 0 in empty slots, whatever those slots held (+-3e20 here): masking goes by id."""
    from acfm_video_3d_reconstruction_amd import ops
    dev = _dev()
    shape = (2, 33, 17)
    c = _soft_case(shape, K, 1e-2)
    b = c.b
    p2f = b.pix_to_face
    filled, empty = p2f >= 0, p2f < 0
    one = ((b.dists == -0.02) & filled).any(-1)
    zero = (((b.dists == 0.02) | empty).all(-1)) & filled.any(-1)
    assert int(one.sum()) > 0 and (int(zero.sum()) > 0 or K > 1)
    dists = b.dists.to(dev).requires_grad_(True)
    out = ops.sigmoid_alpha_blend(None, _frag_tuple(b, dev, dists=dists), _bp(1e-4))
    (gd,) = _grads(out, [dists], c.G.to(dev))
    A, gd = out[..., 3].cpu(), gd.cpu()
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(gd).all())
    assert bool((A[one] == 1.0).all()) and bool((gd[one] == 0).all())
    assert bool((A[zero] == 0.0).all())
    assert bool((A[~filled.any(-1)] == 0.0).all())
    assert bool((gd[empty] == 0).all())
    if K == 1:
        assert bool((A[(b.dists[..., 0] == 0.02) & filled[..., 0]] == 0.0).all())
    # the softmax blend on the same fragments
    dists = b.dists.to(dev).requires_grad_(True)
    zbuf = b.zbuf.to(dev).requires_grad_(True)
    col = c.colors.to(dev).requires_grad_(True)
    out = ops.softmax_rgb_blend(col, _frag_tuple(b, dev, dists=dists, zbuf=zbuf), _bp(1e-2), znear=ZNEAR, zfar=ZFAR)
    grads = [t.cpu() for t in _grads(out, [dists, zbuf, col], c.G.to(dev))]
    assert bool(torch.isfinite(out).all())
    assert bool((out[..., 3].cpu()[one] == 1.0).all())
    for t in grads:
        assert bool(torch.isfinite(t).all()) and bool((t[empty] == 0).all())


# ------------------------------------------------------------------------------ atlas texels
@functools.lru_cache(maxsize=None)
def _atlas_fragments(R, K, shape, F_packed):
    """-> (built fragments with 5 % of the ids >= F_packed, pix_to_face as the reference sees it)."""
    N, H, W = shape
    b = build_fragments(N, H, W, K, 1e-2, _seed(shape, K) + R, F_packed, R=R, over=0.05)
    return b, _mask_over(b.pix_to_face, F_packed)


@gpu
@pytest.mark.parametrize("R,K,shape,ambient,F_packed", ATLAS_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_atlas_texels(R, K, shape, ambient, F_packed):
    """atlas_softmax_blend against float64 with the texel chosen by _texel_index, the float32 torch restatement of
    atlas_texel (the library is built without fused multiply-adds, so the two agree exactly, not approximately).

    Reaches: R = 1, odd R, w R exactly on a grid line, the three corners (w = 1: (int)(w R) = R, caught by the clamp),
    w0 + w1 == 1 (the mirror test <= 1.0f on its boundary), unclipped barycentrics below 0 and above 1; ids >=
    F_packed, which are empty and must not be dereferenced; p / pix_per_mesh changing inside a wave (H W = 63 with
    an ambient [N,3]).  Image, the gradients to atlas, dists and zbuf; then per block (corners, grid lines, diagonal,
    unclipped) the atlas gradient of that block's pixels alone: it meets the reference, is non-zero on every texel
    the reference gives a gradient above 1e-9, and is zero on every texel that no valid slot of the block names.
    For R = 3, F_packed = 3 every texel of face 0 receives gradient."""
    from acfm_video_3d_reconstruction_amd import ops
    dev = _dev()
    N, H, W = shape
    gamma = 1e-2
    b, p2f = _atlas_fragments(R, K, shape, F_packed)
    g = torch.Generator().manual_seed(R * 100 + K)
    atlas = torch.rand(F_packed, R, R, 3, generator=g)
    amb = (0.5 + torch.rand(N, 3, generator=g)) if ambient else None
    G = torch.randn(N, H, W, 4, generator=g)
    ti = _texel_index(p2f, b.bary_coords, R)
    assert int(ti.min()) >= 0 and int(ti.max()) < F_packed * R * R
    rd, rz, ra = _leaf(b.dists), _leaf(b.zbuf), _leaf(atlas)
    colors = ra.reshape(-1, 3)[ti]
    if ambient:
        colors = colors * amb.double()[:, None, None, None, :]
    ref = _ref_softmax(p2f, rd, rz, colors, SIGMA, gamma, BG, ZNEAR, ZFAR)

    dists, zbuf = b.dists.to(dev).requires_grad_(True), b.zbuf.to(dev).requires_grad_(True)
    a = atlas.to(dev).requires_grad_(True)
    img = ops.atlas_softmax_blend(a, _frag_tuple(b, dev, dists=dists, zbuf=zbuf), _bp(gamma),
                                  ambient=amb.to(dev) if ambient else None, znear=ZNEAR, zfar=ZFAR)
    tag = "atlas R=%d K=%d %s ambient=%s" % (R, K, shape, ambient)
    _img(img, ref, what=tag + " image")
    got = _grads(img, [a, dists, zbuf], G.to(dev))
    want = _grads(ref, [ra, rd, rz], G.double())
    _close(got[0], want[0], what=tag + " grad atlas")
    _close(got[1], want[1], what=tag + " grad dists")
    _close(got[2], want[2], what=tag + " grad zbuf")
    over = b.pix_to_face >= F_packed
    assert bool((got[1].cpu()[over] == 0).all()) and bool((got[2].cpu()[over] == 0).all())
    if R == 3 and F_packed == 3 and p2f.numel() > 1000:
        assert bool((got[0][0].abs().amax(-1) > 0).all()), "every texel of face 0"
    valid = p2f >= 0
    for blk, name in ((CORNER, "corners"), (GRID, "grid lines"), (DIAGONAL, "diagonal"), (UNCLIPPED, "unclipped")):
        m = (b.block == blk)
        if not bool((valid & m[..., None]).any()):
            continue
        Gb = G * m[..., None]
        (ga,) = _grads(img, [a], Gb.to(dev))
        (wa,) = _grads(ref, [ra], Gb.double())
        _close(ga, wa, what=tag + " grad atlas, %s" % name)
        nz = (ga.cpu().reshape(-1, 3) != 0).any(-1)
        must = (wa.reshape(-1, 3).abs() > 1e-9).any(-1)
        may = torch.zeros_like(nz)
        may[ti[valid & m[..., None]]] = True
        assert bool((nz | ~must).all()), tag + ": %s: a referenced texel without gradient" % name
        assert bool((may | ~nz).all()), tag + ": %s: gradient on a texel that no slot names" % name


# ------------------------------------------------------------------------------ interpolation
@gpu
@pytest.mark.parametrize("shape,K,D", INTERP_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_interpolate_tails_and_widths(shape, K, D):
    """interpolate_face_attributes at D in {1, 3, 5, 17}, K in {1, 10, 32} and P K no multiple of 256 (the tail of
    k_interp_fwd / k_interp_bwd): through the entry points with out, grad_bary and grad_attrs inside sentinel guards,
    and through the op.  Ids < 0 (-1 and -5) and ids >= F_packed give exactly zero output and zero grad_bary and send
    nothing to the attributes, whatever their barycentrics hold (3e20 here); with every id invalid the attribute
    gradient is exactly zero.  Value bar of test_blends_vs_float64: 1e-6 of sum |b a| plus 1e-7 (unclipped
    barycentrics cancel); gradients at the suite's bars."""
    from acfm_video_3d_reconstruction_amd import _lib, ops
    dev = _dev()
    N, H, W = shape
    P, Fp = N * H * W, 11
    assert (P * K) % 256 != 0
    b = build_fragments(N, H, W, K, 1e-2, _seed(shape, K) + D, Fp, over=0.05)
    p2f = _mask_over(b.pix_to_face, Fp)
    invalid = p2f < 0
    g = torch.Generator().manual_seed(D)
    attrs = torch.randn(Fp, 3, D, generator=g)
    Gi = torch.randn(N, H, W, K, D, generator=g)
    rb, ra = _leaf(b.bary_coords), _leaf(attrs)
    ref = _ref_interp(p2f, rb, ra)
    bound = _ref_interp(p2f, rb.detach().abs(), ra.detach().abs())
    wb, wa = _grads(ref, [rb, ra], Gi.double())
    assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(wb).all()) and bool(torch.isfinite(wa).all())
    tag = "interp %s K=%d D=%d" % (shape, K, D)

    def check(out, gb, ga, how):
        err = (out.detach().double().cpu() - ref.detach()).abs()
        print("%s %s: max err %.3g, max (err - 1e-6 bound) %.3g" % (tag, how, float(err.max()),
                                                                     float((err - 1e-6 * bound).max())))
        assert bool((err <= 1e-6 * bound + 1e-7).all())
        assert bool((out.detach().cpu()[invalid] == 0).all()) and bool((gb.cpu()[invalid] == 0).all())
        _close(gb, wb, what="%s %s grad bary" % (tag, how))
        _close(ga, wa, what="%s %s grad attrs" % (tag, how))

    # the entry points, outputs inside guards
    q = _lib.ptr
    ids, by, fa, go = (t.to(dev).contiguous() for t in (b.pix_to_face, b.bary_coords, attrs, Gi))
    guards = _Guards(dev)
    out, gb, ga = guards(N, H, W, K, D), guards(N, H, W, K, 3), guards(Fp, 3, D)
    _lib.call("acfm_interpolate_face_attributes", dev, q(ids), q(by), q(fa), P, K, Fp, D, q(out), None)
    _lib.call("acfm_interpolate_face_attributes_backward", dev, q(ids), q(by), q(fa), q(go), P, K, Fp, D, q(gb), q(ga),
              None, 0, None)
    guards.check(tag)
    check(out, gb, ga, "entry points")
    # the op
    bary, at = by.clone().requires_grad_(True), fa.clone().requires_grad_(True)
    out = ops.interpolate_face_attributes(ids, bary, at)
    assert out.shape == (N, H, W, K, D)
    gb, ga = _grads(out, [bary, at], go)
    check(out, gb, ga, "op")
    (g1,) = _grads(ops.interpolate_face_attributes(ids, bary, fa), [bary], go)      # grad_attrs NULL
    assert torch.equal(g1, gb)
    # no valid id at all
    none = torch.where(ids >= 0, torch.full_like(ids, Fp + 3), ids)
    out = ops.interpolate_face_attributes(none, bary, at)
    gb, ga = _grads(out, [bary, at], go)
    assert bool((out == 0).all()) and bool((gb == 0).all()) and bool((ga == 0).all())


# ------------------------------------------------------------------------------ contention, deterministic mode
@gpu
def test_scattering_contention_deterministic():
    """Three faces and R = 1: the 1122 x 10 slots of the image add into the atlas' nine floats, and the same ids into
    3 x 3 x 4 attribute gradients -- the heaviest contention the scattering backwards can meet.  Under
    raster_tuning(deterministic=True) two runs are bit-identical and meet the float64 reference at the suite's bars;
    the float atomics of the default mode meet the same bars."""
    from acfm_video_3d_reconstruction_amd import _lib, ops
    dev = _dev()
    shape, K, R, Fp, D, gamma = (2, 33, 17), 10, 1, 3, 4, 1e-2
    N, H, W = shape
    b = build_fragments(N, H, W, K, gamma, 77, Fp, R=R, over=0.05)
    p2f = _mask_over(b.pix_to_face, Fp)
    g = torch.Generator().manual_seed(77)
    atlas, attrs = torch.rand(Fp, R, R, 3, generator=g), torch.randn(Fp, 3, D, generator=g)
    G, Gi = torch.randn(N, H, W, 4, generator=g), torch.randn(N, H, W, K, D, generator=g)
    ra, rf = _leaf(atlas), _leaf(attrs)
    ti = _texel_index(p2f, b.bary_coords, R)
    ref = _ref_softmax(p2f, b.dists.double(), b.zbuf.double(), ra.reshape(-1, 3)[ti], SIGMA, gamma, BG, ZNEAR, ZFAR)
    (wa,) = _grads(ref, [ra], G.double())
    (wf,) = _grads(_ref_interp(p2f, b.bary_coords.double(), rf), [rf], Gi.double())
    frag = _frag_tuple(b, dev)

    def grads():
        a, fa = atlas.to(dev).requires_grad_(True), attrs.to(dev).requires_grad_(True)
        img = ops.atlas_softmax_blend(a, frag, _bp(gamma), znear=ZNEAR, zfar=ZFAR)
        out = ops.interpolate_face_attributes(frag[0], frag[2], fa)
        return torch.autograd.grad([img, out], [a, fa], [G.to(dev), Gi.to(dev)])

    with _lib.raster_tuning(deterministic=True):
        x, y = grads(), grads()
    z = grads()
    for u, v in zip(x, y):
        assert torch.equal(u, v)
    for how, (ga, gf) in (("deterministic", x), ("atomics", z)):
        _close(ga, wa, what="contention, %s: grad atlas" % how)
        _close(gf, wf, what="contention, %s: grad attrs" % how)
