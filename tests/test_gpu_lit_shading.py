"""GPU: the lit kernels (csrc/acfm_light.hip) through ops.vertex_normals, ops.light_points and ops.phong_shade, and
the shim's shading functions and shaders on top of them, against the float64 restatements of lit_reference.py and
against the composition of torch operators (shading.fused(False)).  Bars: the project's, 1e-4 of scale and 1e-5
relative L2 (2e-5 for the vertex gradient at shininess 64), 1e-6 for the normals themselves."""
import numpy as np
import pytest
import torch

import lit_reference as R
from test_gpu_shaders import SIL_BLUR, _dev, _scene, _vertex_colour_scene

pytestmark = pytest.mark.gpu


def _leaf(t, d=None):
    t = t.detach().clone()
    return (t.to(d) if d is not None else t.double().cpu()).requires_grad_(True)


def _sphere(n, seed, jitter=0.05):
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.utils import ico_sphere
    s = ico_sphere(1)
    v0, f = s.verts_packed().cpu(), s.faces_packed().cpu()
    g = torch.Generator().manual_seed(seed)
    verts = (v0[None] + jitter * torch.randn(n, v0.shape[0], 3, generator=g)).float()
    return verts.reshape(-1, 3), torch.cat([f + i * v0.shape[0] for i in range(n)], 0)


# ------------------------------------------------------------------------------------------------ ops.vertex_normals
def _normal_mesh(name, meshes):
    if name == "tetrahedron":
        return (torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]),
                torch.tensor([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]]))
    if name == "spheres":
        return _sphere(3, 5)
    if name == "fan":
        return R.fan(64)
    if name == "degenerate":
        # face 2 has zero area (collinear, exactly), vertices 5 and 6 coincide and span face 3 (zero area as well),
        # vertex 7 is in no face; vertices 4, 5, 6 touch zero-area faces only: their normals are exactly 0
        v = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [3, 0, 0], [1, 1, 1], [1, 1, 1], [5, 5, 5]])
        return v, torch.tensor([[0, 1, 2], [1, 3, 2], [1, 3, 4], [4, 5, 6]])
    v, f = meshes["horse_v"], meshes["horse_f"]
    g = torch.Generator().manual_seed(6)
    verts = torch.from_numpy(v).float()[None] + 0.01 * torch.randn(2, v.shape[0], 3, generator=g)
    f = torch.from_numpy(np.ascontiguousarray(f)).long()
    return verts.reshape(-1, 3), torch.cat([f, f + v.shape[0]], 0)


@pytest.mark.parametrize("name", ["tetrahedron", "spheres", "fan", "degenerate", "horses"])
def test_vertex_normals_vs_float64(meshes, name):
    from acfm_video_3d_reconstruction_amd import ops
    d = _dev()
    verts, faces = _normal_mesh(name, meshes)
    V, F = verts.shape[0], faces.shape[0]
    if name == "fan":
        assert V == 65
    if name == "horses":
        assert V == 2 * 642
    table = ops.incidence_table(faces.to(d), V)
    g = torch.Generator().manual_seed(1)
    Gv, Gf = torch.randn(V, 3, generator=g), torch.randn(F, 3, generator=g)

    def run():
        v = _leaf(verts, d)
        vn, fn = ops.vertex_normals(v, faces.to(d), table)
        gboth, = torch.autograd.grad((vn * Gv.to(d)).sum() + (fn * Gf.to(d)).sum(), v, retain_graph=True)
        gvn, = torch.autograd.grad((vn * Gv.to(d)).sum(), v, retain_graph=True)
        gfn, = torch.autograd.grad((fn * Gf.to(d)).sum(), v)
        return vn, fn, gboth, gvn, gfn

    got, again = run(), run()
    for a, b in zip(got, again):
        assert torch.equal(a, b)
    rv = _leaf(verts)
    rvn, rfn = R.normals(rv, faces)
    for a, r, what in ((got[0], rvn, "vertex normals"), (got[1], rfn, "face normals")):
        assert bool(torch.isfinite(a).all())
        err = float((a.double().cpu() - r.detach()).abs().max())
        print("%s %s: max err %.3g" % (name, what, err))
        assert err <= 1e-6, (what, err)
    if name == "degenerate":
        assert bool((got[0][4:] == 0).all()) and bool((got[1][2:] == 0).all())
    refs = (torch.autograd.grad((rvn * Gv.double()).sum() + (rfn * Gf.double()).sum(), rv, retain_graph=True)[0],
            torch.autograd.grad((rvn * Gv.double()).sum(), rv, retain_graph=True)[0],
            torch.autograd.grad((rfn * Gf.double()).sum(), rv)[0])
    for a, r, what in zip(got[2:], refs, ("both", "vertex normals", "face normals")):
        R.close(a, r, floor=1e-6, what="%s grad verts through %s" % (name, what))


# ------------------------------------------------------------------------------------------------ ops.phong_shade
AMB = ((0.3, 0.25, 0.2), (0.1, 0.2, 0.3))
DIF = ((0.6, 0.5, 0.4), (0.3, 0.7, 0.5))
SPEC = ((0.5, 0.4, 0.45), (0.2, 0.3, 0.6))
VEC = {False: ((0.3, 1.0, -1.0), (-0.5, 0.4, -1.0)), True: ((0.5, 1.0, -2.0), (-1.0, 0.3, -1.5))}
CAM = ((0.0, 0.0, -2.732), (0.4, -0.2, -3.0))


def _light(N, point, shin, per_mesh, d):
    """-> (ops.LightConstants, lit_reference.Light): colours and vectors [1,3] or [N,3], shininess a number or [N]."""
    from acfm_video_3d_reconstruction_amd import ops
    rows = lambda t: torch.tensor(t[:N] if per_mesh else t[:1])
    parts = [rows(AMB), rows(DIF), rows(SPEC), rows(VEC[point]), rows(CAM)]
    lc = ops.light_constants(*[p.to(d) for p in parts], shin.to(d) if torch.is_tensor(shin) else shin, N, point)
    return lc, R.Light(N, *parts[:4], point, parts[4], shin)


def _shade_case(shape, K, mode, point, shin, per_mesh, d, bary_grad=True):
    """Both sides of one ops.phong_shade case on hand-built fragments over jittered ico-spheres."""
    from acfm_video_3d_reconstruction_amd import ops
    N, H, W = shape
    verts, faces = _sphere(N, 11 * K + H)
    Fm = faces.shape[0] // N
    p2f, zbuf, bary, dists, g = R.fragments(N, H, W, K, Fm, 100 * K + H + W)
    texels = torch.rand(N, H, W, K, 3, generator=g)
    G = torch.randn(N, H, W, K, 3, generator=g)
    if torch.is_tensor(shin):
        shin = shin[:N]
    lc, ref_light = _light(N, point, shin, per_mesh, d)
    v, t, b = _leaf(verts, d), _leaf(texels, d), bary.to(d).requires_grad_(bary_grad)
    table = ops.incidence_table(faces.to(d), verts.shape[0])
    vn, fn = ops.vertex_normals(v, faces.to(d), table)
    frag = (p2f.to(d), zbuf.to(d), b, dists.to(d))
    col = ops.phong_shade(frag, v, faces.to(d), vn if mode == "phong" else fn, t, lc, table, mode=mode)
    leaves = (t, v, b) if bary_grad and mode == "phong" else (t, v)
    grads = torch.autograd.grad((col * G.to(d)).sum(), leaves)
    rv, rt, rb = _leaf(verts), _leaf(texels), _leaf(bary)
    ref = R.shade(mode, rv, faces, p2f, rb, rt, ref_light)
    rgrads = torch.autograd.grad((ref * G.double()).sum(), (rt, rv, rb)[:len(leaves)])
    return col, grads, ref, rgrads


def _check_shade(col, grads, ref, rgrads, shin, what):
    R.close(col, ref, floor=0.0, what=what + " colours")
    big = float(torch.as_tensor(shin).max()) >= 64
    for gr, rr, name in zip(grads, rgrads, ("texels", "verts", "bary")):
        R.close(gr, rr, floor=1e-9 if name == "texels" else 1e-6, what="%s grad %s" % (what, name),
                rel_l2=2e-5 if name == "verts" and big else 1e-5)


SHAPES = [(1, 1, 1), (1, 5, 13), (2, 9, 9)]
SHININESS = [1, 10, 64, torch.tensor([10.0, 64.0]), torch.tensor([1.0, 3.0])]


@pytest.mark.parametrize("point", [False, True], ids=["directional", "point"])
@pytest.mark.parametrize("mode", ["phong", "flat"])
@pytest.mark.parametrize("K", [1, 8, 20])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_phong_shade_vs_float64(shape, K, mode, point):
    """Every (shape, K, mode, light kind); the shininess (1, 10, 64 as a number, and per mesh) and the constants'
    shapes ([1,3] / [N,3]) cycle over the cases so that each value meets each mode and light kind."""
    d = _dev()
    i = SHAPES.index(shape) + [1, 8, 20].index(K) + (mode == "flat") + 2 * point
    for shin, per_mesh in ((SHININESS[i % 3], bool(i % 2)), (SHININESS[3 + i % 2], True)):
        col, grads, ref, rgrads = _shade_case(shape, K, mode, point, shin, per_mesh, d)
        _check_shade(col, grads, ref, rgrads, shin, "%s K%d %s point=%d s=%s" % (shape, K, mode, point, shin))


@pytest.mark.parametrize("shin", [1, 64])
def test_phong_shade_constructed_slots(shin):
    """One face per image, each with its own directional light: the normal exactly perpendicular to the light
    (cos == 0), the light behind the face, a lit face with v.r <= 0, and vertex normals that cancel (the interpolated
    normal is exactly 0, shorter than the 1e-6 of the normalisation); then an ordinary lit face as the control.  Each
    is finite and equals the restatement, gradients included."""
    from acfm_video_3d_reconstruction_amd import ops
    d = _dev()
    N = 5
    tri = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])
    verts = torch.cat([tri + 0.1 * n for n in range(N)], 0)
    faces = torch.arange(3 * N).reshape(N, 3)
    up = torch.tensor([0.0, 0.0, 1.0])
    normals = up.repeat(3 * N, 1)
    normals[3:6] = -up                              # image 1: the light (0, 0, 1) is behind the face
    normals[10] = -up                               # image 3: with bary (0.5, 0.5, 0) the normals cancel exactly
    vec = torch.tensor([[1.0, 0, 0], [0, 0, 1.0], [1.0, 0, 0.1], [0.3, 0.2, 1.0], [0.3, 0.2, 1.0]])
    cam = torch.tensor([[0.0, 0, 5], [0, 0, 5], [10.0, 0, 0.05], [0, 0, 5], [0.2, 0.1, 5]])
    bary = torch.tensor([[0.2, 0.3, 0.5], [0.2, 0.3, 0.5], [0.2, 0.3, 0.5], [0.5, 0.5, 0.0], [0.2, 0.3, 0.5]])
    p2f = torch.arange(N).reshape(N, 1, 1, 1)
    g = torch.Generator().manual_seed(3)
    texels, G = torch.rand(N, 1, 1, 1, 3, generator=g), torch.randn(N, 1, 1, 1, 3, generator=g)
    parts = [torch.tensor(AMB[:1]), torch.tensor(DIF[:1]), torch.tensor(SPEC[:1]), vec, cam]
    lc = ops.light_constants(*[p.to(d) for p in parts], shin, N, False)
    ref_light = R.Light(N, *parts[:4], False, cam, shin)
    table = ops.incidence_table(faces.to(d), 3 * N)
    v, n, t = _leaf(verts, d), _leaf(normals, d), _leaf(texels, d)
    b = bary.reshape(N, 1, 1, 1, 3).to(d).requires_grad_(True)
    plane = torch.zeros(N, 1, 1, 1, device=d)
    col = ops.phong_shade((p2f.to(d), plane, b, plane), v, faces.to(d), n, t, lc, table)
    grads = torch.autograd.grad((col * G.to(d)).sum(), (t, v, n, b))
    rv, rn, rt, rb = _leaf(verts), _leaf(normals), _leaf(texels), _leaf(bary.reshape(N, 1, 1, 1, 3))
    c, s = ref_light.at(5)
    pos, nrm = R.interpolate(p2f, rb, rv[faces]), R.interpolate(p2f, rb, rn[faces])
    ref = R.lighting(pos, nrm, rt, c["amb"], c["dif"], c["spec"], c["vec"], False, c["cam"], s)
    rgrads = torch.autograd.grad((ref * G.double()).sum(), (rt, rv, rn, rb))
    # what the construction is for: no diffuse and no specular light in images 0, 1 and 3, no specular in image 2
    amb_only = torch.tensor(AMB[0], dtype=torch.float64) * rt.detach()
    for i in (0, 1, 3):
        assert torch.allclose(ref[i].detach(), amb_only[i], atol=1e-12), i
    assert float((ref[4].detach() - amb_only[4]).abs().max()) > 1e-2
    R.close(col, ref, floor=0.0, what="constructed colours")
    for gr, rr, name in zip(grads, rgrads, ("texels", "verts", "normals", "bary")):
        R.close(gr, rr, floor=1e-9, what="constructed grad " + name)


def test_light_points_vs_float64():
    """Gouraud's vertex stage: 2 meshes of 42 points (84: one wave and a part of the next), per-mesh constants and
    shininess (10 and 64), both light kinds.  The gradients to points and normals run back through relu(v.r)^64 in
    float32 like the vertex gradient of phong_shade, and take its bar at shininess 64 (2e-5 relative L2); the colour
    gradient does not pass the power and keeps 1e-5."""
    from acfm_video_3d_reconstruction_amd import ops
    d = _dev()
    N = 2
    verts, faces = _sphere(N, 8)
    M = verts.shape[0]
    g = torch.Generator().manual_seed(9)
    nrm, col, G = torch.randn(M, 3, generator=g), torch.rand(M, 3, generator=g), torch.randn(M, 3, generator=g)
    idx = torch.arange(N).repeat_interleave(M // N)
    for point in (False, True):
        lc, ref_light = _light(N, point, torch.tensor([10.0, 64.0]), True, d)
        p, n, c = _leaf(verts, d), _leaf(nrm, d), _leaf(col, d)
        out = ops.light_points(p, n, c, lc, idx.to(d))
        grads = torch.autograd.grad((out * G.to(d)).sum(), (p, n, c))
        rp, rn, rc = _leaf(verts), _leaf(nrm), _leaf(col)
        k, s = ref_light.at(3)
        sh = lambda t: t.reshape(N, M // N, 3)
        ref = R.lighting(sh(rp), sh(rn), sh(rc), k["amb"], k["dif"], k["spec"], k["vec"], point, k["cam"], s)
        rgrads = torch.autograd.grad((ref * sh(G.double())).sum(), (rp, rn, rc))
        R.close(out, ref.reshape(M, 3), floor=0.0, what="light_points point=%d" % point)
        for gr, rr, name in zip(grads, rgrads, ("points", "normals", "colours")):
            R.close(gr, rr, floor=1e-9, what="light_points grad " + name, rel_l2=1e-5 if name == "colours" else 2e-5)


# ------------------------------------------------------------------------------------------------ contention
def test_one_face_in_every_slot():
    """N = 1, 16 x 16, K = 8, all 2048 slots on one face: every corner sum has 2048 addends.  Default mode (float
    atomics behind the in-wave sums) and deterministic mode are within the bars; deterministic mode gives the same bits
    twice."""
    from acfm_video_3d_reconstruction_amd import _lib, ops
    d = _dev()
    H, K = 16, 8
    verts, faces = _sphere(1, 12)
    p2f, zbuf, bary, dists, g = R.fragments(1, H, H, K, faces.shape[0], 13)
    p2f = torch.full_like(p2f, 7)
    texels, G = torch.rand(1, H, H, K, 3, generator=g), torch.randn(1, H, H, K, 3, generator=g)
    lc, ref_light = _light(1, True, 10, False, d)
    table = ops.incidence_table(faces.to(d), verts.shape[0])

    def run():
        v, t = _leaf(verts, d), _leaf(texels, d)
        vn, _ = ops.vertex_normals(v, faces.to(d), table)
        col = ops.phong_shade((p2f.to(d), zbuf.to(d), bary.to(d), dists.to(d)), v, faces.to(d), vn, t, lc, table)
        return torch.autograd.grad((col * G.to(d)).sum(), (t, v))

    rv, rt = _leaf(verts), _leaf(texels)
    ref = R.shade("phong", rv, faces, p2f, bary.double(), rt, ref_light)
    rgrads = torch.autograd.grad((ref * G.double()).sum(), (rt, rv))
    for gr, rr, name in zip(run(), rgrads, ("texels", "verts")):
        R.close(gr, rr, floor=1e-6, what="one face, default mode, grad " + name)
    with _lib.raster_tuning(deterministic=True):
        x, y = run(), run()
    for a, b, rr, name in zip(x, y, rgrads, ("texels", "verts")):
        assert torch.equal(a, b), name
        R.close(a, rr, floor=1e-6, what="one face, deterministic mode, grad " + name)


# ------------------------------------------------------------------------------------------------ dispatch
class _Spy:
    def __init__(self, monkeypatch):
        from acfm_video_3d_reconstruction_amd import _lib
        self.names, real = [], _lib.call

        def call(name, *a, **k):
            self.names.append(name)
            return real(name, *a, **k)
        monkeypatch.setattr(_lib, "call", call)

    def take(self):
        out, self.names = self.names, []
        return out


def _atlas_scene(meshes, d, n=2, H=32, K=8, R_=3, seed=103):
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.renderer import (MeshRasterizer, RasterizationSettings,
                                                                          SfMOrthographicCameras, TexturesAtlas)
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.structures import Meshes
    vs, f, Rm, T, _ = _vertex_colour_scene(meshes, n, seed)
    cameras = SfMOrthographicCameras(device=d)
    rast = MeshRasterizer(cameras=cameras, raster_settings=RasterizationSettings(
        image_size=H, blur_radius=SIL_BLUR, faces_per_pixel=K, clip_barycentric_coords=True))
    atlas = torch.rand(n, f.shape[0], R_, R_, 3, device=d, generator=torch.Generator(device=d).manual_seed(seed))
    mesh = Meshes(verts=vs, faces=f[None].expand(n, -1, -1), textures=TexturesAtlas(atlas))
    return mesh, rast(mesh, R=Rm, T=T), cameras, dict(R=Rm, T=T)


def test_dispatch(meshes, monkeypatch):
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.renderer import (BlendParams, DirectionalLights,
                                                                          HardPhongShader, SoftPhongShader)
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.renderer.mesh import shading
    d = _dev()
    mesh, fr, cameras, view = _atlas_scene(meshes, d)
    kw = dict(ambient_color=((0.3, 0.3, 0.3),), specular_color=((0.5, 0.5, 0.5),), direction=((0.3, 1.0, -1.0),))
    lit = DirectionalLights(diffuse_color=((0.6, 0.5, 0.4),), device=d, **kw)
    mesh.verts_normals_packed()                      # (its kernel is not what is counted below)
    spy = _Spy(monkeypatch)
    for cls in (SoftPhongShader, HardPhongShader):
        shader = cls(device=d, cameras=cameras, lights=lit, blend_params=BlendParams(1e-4, 1e-2, 0))
        fused = shader(fr, mesh, **view)
        names = spy.take()
        assert "acfm_phong_shade" in names and "acfm_interpolate_face_attributes" not in names, names
        with shading.fused(False):
            plain = shader(fr, mesh, **view)
        names = spy.take()
        assert "acfm_phong_shade" not in names and names.count("acfm_interpolate_face_attributes") == 2, names
        R.close(fused, plain.double(), floor=0.0, what=cls.__name__ + " fused against the composition")
        # a light colour that requires a gradient: the composition, and the gradient arrives
        colour = torch.tensor([[0.6, 0.5, 0.4]], device=d, requires_grad=True)
        learn = DirectionalLights(diffuse_color=colour, device=d, **kw)
        learn.diffuse_color = colour
        img = shader(fr, mesh, lights=learn, **view)
        names = spy.take()
        assert "acfm_phong_shade" not in names and names.count("acfm_interpolate_face_attributes") == 2, names
        g, = torch.autograd.grad(img[..., :3].sum(), colour)
        assert float(g.abs().max()) > 0
    # the reference's configuration: ambient only + TexturesAtlas -> the atlas blend, the same bits either way
    amb = DirectionalLights(ambient_color=((0.8, 0.9, 1.0),), diffuse_color=((0.0, 0.0, 0.0),),
                            specular_color=((0.0, 0.0, 0.0),), device=d)
    shader = SoftPhongShader(device=d, cameras=cameras, lights=amb, blend_params=BlendParams(1e-4, 1e-2, 0))
    a = shader(fr, mesh, **view)
    names = spy.take()
    assert names == ["acfm_softmax_rgb_blend"], names
    with shading.fused(False):
        b = shader(fr, mesh, **view)
    assert spy.take() == ["acfm_softmax_rgb_blend"] and torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ end to end
SHADERS = ["SoftPhongShader", "HardPhongShader", "SoftGouraudShader", "HardGouraudShader", "HardFlatShader"]


@pytest.mark.parametrize("point", [False, True], ids=["directional", "point"])
@pytest.mark.parametrize("name", SHADERS)
def test_renderer_fused_against_composition(meshes, name, point):
    """MeshRenderer with each lit shader on 2 horses, 64 x 64, K = 8, vertex colours: the fused kernels against the
    composition of torch operators on the same fragments; images, vertex and colour gradients."""
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim import renderer as PR
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.renderer.mesh import shading
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.structures import Meshes
    d = _dev()
    n, H, K = 2, 64, 8
    vs, f, Rm, T, rgb = _vertex_colour_scene(meshes, n, 110 + point)
    assert not (Rm.requires_grad or T.requires_grad)       # (else both sides would run the composition)
    kw = dict(ambient_color=((0.3, 0.3, 0.3),), diffuse_color=((0.6, 0.5, 0.4),), specular_color=((0.5, 0.5, 0.5),))
    lights = PR.PointLights(location=((0.5, 1.0, -2.0),), device=d, **kw) if point else \
        PR.DirectionalLights(direction=((0.3, 1.0, -1.0),), device=d, **kw)
    cameras = PR.SfMOrthographicCameras(device=d)
    renderer = PR.MeshRenderer(
        rasterizer=PR.MeshRasterizer(cameras=cameras, raster_settings=PR.RasterizationSettings(
            image_size=H, blur_radius=SIL_BLUR, faces_per_pixel=K, clip_barycentric_coords=True)),
        shader=getattr(PR, name)(device=d, cameras=cameras, lights=lights, materials=PR.Materials(device=d, shininess=10),
                                 blend_params=PR.BlendParams(1e-4, 1e-2, (0.1, 0.2, 0.3))))
    G = None
    out = {}
    for on in (True, False):
        v, c = vs.clone().requires_grad_(True), rgb.clone().requires_grad_(True)
        mesh = Meshes(verts=v, faces=f[None].expand(n, -1, -1), textures=PR.Textures(verts_rgb=c))
        fr = renderer.rasterizer(mesh, R=Rm, T=T)
        fr = fr._replace(**{k: getattr(fr, k).detach() for k in ("zbuf", "bary_coords", "dists")})
        with shading.fused(on):
            img = renderer.shader(fr, mesh, R=Rm, T=T)
        G = torch.randn(img.shape, device=d, generator=torch.Generator(device=d).manual_seed(1)) if G is None else G
        out[on] = (img,) + torch.autograd.grad((img * G).sum(), (v, c))
    assert 0.05 < float((fr.pix_to_face[..., 0] >= 0).float().mean()) < 0.95
    for a, b, what in zip(out[True], out[False], ("image", "grad verts", "grad colours")):
        R.close(a, b.double(), floor=0.0 if what == "image" else 1e-6, what="%s %s" % (name, what))


# ------------------------------------------------------------------------------------------------ hipGraph
def test_soft_phong_graph_capture(meshes):
    """Forward + backward of SoftPhongShader with a point light (2 horses, 64 x 64, K = 8) captured into a hipGraph and
    replayed twice with new vertices: in deterministic mode the replay equals the eager run bit for bit."""
    from acfm_video_3d_reconstruction_amd import _lib, ops
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim import renderer as PR
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.structures import Meshes
    d = _dev()
    n, H, K = 2, 64, 8
    ndc, f = _scene(meshes, "horse", n, 120)
    first = torch.tensor(ndc, device=d)
    later = first + 0.01 * torch.randn(first.shape, device=d, generator=torch.Generator(device=d).manual_seed(2))
    tv = first.clone().requires_grad_(True)
    faces = torch.from_numpy(f).to(d)[None].expand(n, -1, -1).contiguous()
    rgb = torch.rand(n, first.shape[1], 3, device=d)
    G = torch.rand(n, H, H, 4, device=d)
    cameras = PR.SfMOrthographicCameras(device=d, T=torch.tensor([[0.0, 0.0, 2.732]]))
    lights = PR.PointLights(location=((0.5, 1.0, -2.0),), ambient_color=((0.3, 0.3, 0.3),),
                            diffuse_color=((0.6, 0.5, 0.4),), specular_color=((0.5, 0.5, 0.5),), device=d)
    shader = PR.SoftPhongShader(device=d, cameras=cameras, lights=lights, materials=PR.Materials(device=d, shininess=10),
                                blend_params=PR.BlendParams(1e-4, 1e-2, 0))

    def step():
        with _lib.raster_tuning(deterministic=True):
            fr = PR.Fragments(*ops.rasterize_fragments(tv, faces, H, K, blur_radius=SIL_BLUR,
                                                       clip_barycentric_coords=True))
            mesh = Meshes(verts=tv, faces=faces, textures=PR.Textures(verts_rgb=rgb))
            img = shader(fr, mesh)
            return (img,) + torch.autograd.grad((img * G).sum(), (tv,))

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = step()
    with torch.no_grad():
        tv.copy_(later)
    for _ in range(2):
        ops.graph_replay(g)
    torch.cuda.synchronize()
    got = [t.detach().clone() for t in outs]
    ref = [t.detach() for t in step()]
    assert float(ref[1].abs().max()) > 0
    for a, b, what in zip(got, ref, ("image", "grad verts")):
        assert torch.equal(a, b), what


# ------------------------------------------------------------------------------------------------ VisRenderer
def test_vis_renderer(meshes):
    """Unlit, a call is the NeuralRenderer texture render clipped to uint8, exactly; after set_light_dir it is the
    explicit MeshRenderer + DirectionalLights + SoftPhongShader composition in the reference's view, within one grey
    level, and no longer the flat image."""
    from acfm_video_3d_reconstruction_amd import ops, vis
    from acfm_video_3d_reconstruction_amd.nnutils.nmr import NeuralRenderer
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim import renderer as PR
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.structures import Meshes
    d = _dev()
    H = 64
    v = torch.tensor(meshes["bird_v"], dtype=torch.float32, device=d)
    v = v / float(v.abs().max())
    f = torch.from_numpy(np.ascontiguousarray(meshes["bird_f"])).to(d)
    cam = torch.tensor([0.8, 0.05, -0.1, 0.9, 0.3, -0.2, 0.1], device=d)
    cam[3:] /= cam[3:].norm()
    r = vis.VisRenderer(H, f.cpu().numpy())
    colour = torch.tensor(vis.DEFAULT_COLOUR, device=d).expand(1, v.shape[0], 3).contiguous()

    def u8(img):                                   # [3,H,W] float -> uint8 [H,W,3] the viewer's way
        return (img.permute(1, 2, 0).clamp(0, 1) * 255.0).cpu().numpy().astype(np.uint8)

    flat = r(v, cam)
    assert flat.dtype == np.uint8 and flat.shape == (H, H, 3)
    want = NeuralRenderer(H).forward(v[None], f[None], cam[None], colour, atlas=False)[0][0]
    assert np.array_equal(flat, u8(want))
    covered = flat.reshape(-1, 3).any(axis=1)
    assert 0.05 < covered.mean() < 0.95
    atlas = torch.rand(f.shape[0], 2, 2, 3, device=d, generator=torch.Generator(device=d).manual_seed(4))
    want = NeuralRenderer(H).forward(v[None], f[None], cam[None], atlas[None], atlas=True)[0][0]
    assert np.array_equal(r(v, cam, texture=atlas), u8(want))
    assert r.rotated(v, 30).shape == (H, H, 3)
    img, kps = r.diff_vp(v, cam, angle=45, axis=[0, 1, 0], kp_verts=v[:5])
    assert img.shape == (H, H, 3) and kps.shape == (5, 2)

    direction, int_dir, int_amb = [0.3, 1.0, -1.0], 0.7, 0.4
    r.set_light_dir(direction, int_dir, int_amb)
    lit = r(v, cam)
    vs = ops.project(v[None], cam[None]) * torch.tensor([1.0, -1.0, 1.0], device=d)
    Rm, T = PR.look_at_view_transform(eye=((0, 0, -2.732),), device=d)
    Rm[:, 0, 0] *= -1
    cameras = PR.SfMOrthographicCameras(device=d)
    lights = PR.DirectionalLights(ambient_color=((int_amb,) * 3,), diffuse_color=((int_dir,) * 3,),
                                  specular_color=((0.0, 0.0, 0.0),), direction=(direction,), device=d)
    explicit = PR.MeshRenderer(
        rasterizer=PR.MeshRasterizer(cameras=cameras, raster_settings=PR.RasterizationSettings(
            image_size=H, blur_radius=0.0, faces_per_pixel=1, clip_barycentric_coords=True)),
        shader=PR.SoftPhongShader(device=d, cameras=cameras, lights=lights,
                                  blend_params=PR.BlendParams(background_color=0)))
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.renderer.mesh import shading
    with shading.fused(False), torch.no_grad():
        ref = explicit(Meshes(verts=vs, faces=f[None], textures=PR.Textures(verts_rgb=colour)), R=Rm.to(d), T=T.to(d))
    ref = u8(ref[0, ..., :3].permute(2, 0, 1))
    assert int(np.abs(lit.astype(np.int32) - ref.astype(np.int32)).max()) <= 1
    assert int(np.abs(lit.astype(np.int32) - flat.astype(np.int32)).max()) > 20
    r.set_light_dir(None)
    assert np.array_equal(r(v, cam), flat)
