"""GPU: the lit kernels (csrc/acfm_light.hip) on hostile, fenced memory (tests/guards.py run_case) through their public
operators: nothing is written outside the outputs, every output element and workspace word the results depend on is
written, and the bits are the same over both poison patterns and with fenced inputs.  The scattering shader backward
runs in the fixed-point mode (_lib.raster_tuning(deterministic=True)), whose workspace is poisoned here."""
import pytest
import torch

import guards
import lit_reference as R
from test_gpu_guards_other import SHADE_SHAPES, _d, _fragments, _leaf

pytestmark = pytest.mark.gpu
_report = guards.module_report(__name__)


def _mesh(kind, N):
    """-> (verts [V,3], faces [F,3]) packed: `N` 7-face strips over 9 vertices each, or the 65-vertex fan."""
    if kind == "fan":
        return R.fan(64)
    g = torch.Generator().manual_seed(5)
    v = torch.rand(N * 9, 3, generator=g)
    f = torch.stack([torch.arange(7), torch.arange(7) + 1, torch.arange(7) + 2], 1)
    return v, torch.cat([f + 9 * n for n in range(N)], 0)


def _consts(N, point, d):
    from acfm_video_3d_reconstruction_amd import ops
    g = torch.Generator().manual_seed(6)
    parts = [torch.rand(N, 3, generator=g).to(d) for _ in range(3)]
    parts += [(torch.rand(N, 3, generator=g) - 0.5).to(d), torch.tensor([[0.2, 0.1, -3.0]], device=d)]
    return ops.light_constants(*parts, torch.tensor([3.0, 10.0, 64.0])[:N].to(d), N, point)


@pytest.mark.parametrize("kind", ["strip", "fan"])
def test_vertex_normals(kind):
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    verts, faces = _mesh(kind, 1)
    g = torch.Generator().manual_seed(1)
    Gv, Gf = torch.randn(verts.shape[0], 3, generator=g), torch.randn(faces.shape[0], 3, generator=g)

    def fn(inp):
        v = inp(_leaf(verts, d))
        table = ops.incidence_table(faces.to(d), verts.shape[0])
        vn, fnorm = ops.vertex_normals(v, faces.to(d), table)
        gboth, = torch.autograd.grad((vn * inp(Gv.to(d))).sum() + (fnorm * inp(Gf.to(d))).sum(), v, retain_graph=True)
        gf, = torch.autograd.grad((fnorm * inp(Gf.to(d))).sum(), v)
        return dict(vn=vn, fn=fnorm, gboth=gboth, gf=gf)
    guards.run_case(fn)


@pytest.mark.parametrize("point", [False, True], ids=["directional", "point"])
@pytest.mark.parametrize("kind", ["strip", "fan"])
def test_light_points(kind, point):
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    N = 1 if kind == "fan" else 3
    verts, _ = _mesh(kind, N)
    M = verts.shape[0]
    g = torch.Generator().manual_seed(2)
    nrm, col, G = torch.randn(M, 3, generator=g), torch.rand(M, 3, generator=g), torch.randn(M, 3, generator=g)
    idx = torch.arange(N).repeat_interleave(M // N).to(d)

    def fn(inp):
        p, n, c = inp(_leaf(verts, d)), inp(_leaf(nrm, d)), inp(_leaf(col, d))
        out = ops.light_points(p, n, c, _consts(N, point, d), idx)
        gp, gn, gc = torch.autograd.grad(out, (p, n, c), inp(G.to(d)))
        return dict(out=out, gp=gp, gn=gn, gc=gc)
    guards.run_case(fn)


@pytest.mark.parametrize("mode", ["phong", "flat"])
@pytest.mark.parametrize("shape", SHADE_SHAPES + ["fan"], ids=str)
def test_phong_shade(shape, mode):
    """Forward and backward (texels, barycentrics, verts and normals) in deterministic mode: at P = 1 and P = 65 on
    7-face strips, and with the 65-vertex fan (a hub of valence 64 in the corner gather) under 5 x 13 pixels."""
    from acfm_video_3d_reconstruction_amd import _lib, ops
    d = _d()
    N, H, W = (1, 5, 13) if shape == "fan" else shape
    K = 2
    verts, faces = _mesh("fan" if shape == "fan" else "strip", N)
    Fm = faces.shape[0] // N
    p2f, zbuf, bary, dists, g = _fragments(N, H, W, K, Fm, 7)
    texels = torch.rand(N, H, W, K, 3, generator=g)
    G = torch.randn(N, H, W, K, 3, generator=g)
    rows = faces.shape[0] if mode == "flat" else verts.shape[0]
    nrm = torch.randn(rows, 3, generator=g)

    def fn(inp):
        v, n, t, b = inp(_leaf(verts, d)), inp(_leaf(nrm, d)), inp(_leaf(texels, d)), inp(_leaf(bary, d))
        table = ops.incidence_table(faces.to(d), verts.shape[0])
        with _lib.raster_tuning(deterministic=True):
            out = ops.phong_shade((p2f.to(d), inp(zbuf.to(d)), b, inp(dists.to(d))), v, faces.to(d), n, t,
                                  _consts(N, True, d), table, mode=mode)
            leaves = (v, n, t, b) if mode == "phong" else (v, n, t)
            grads = torch.autograd.grad(out, leaves, inp(G.to(d)))
        return dict(out=out, **{"g%d" % i: x for i, x in enumerate(grads)})
    guards.run_case(fn)
