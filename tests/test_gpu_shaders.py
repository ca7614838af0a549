"""GPU: the shaders over fragments (ops.sigmoid_alpha_blend / softmax_rgb_blend / atlas_softmax_blend /
interpolate_face_attributes and the pytorch3d_shim shaders) against float64 torch restatements of SURVEY App-A.5, A.6,
A.10 and against the fused renders.  Bars: images 1e-6; gradients 1e-4 of their scale and 1e-5 relative L2."""
import math

import numpy as np
import pytest
import torch

from helpers import batch_verts, make_cams  # noqa: F401
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SIL_BLUR = math.log(1.0 / 1e-4 - 1.0) * 1e-4
EPS = 1e-10


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _scene(meshes, name, n, seed, shift=0.0):
    rng = np.random.default_rng(seed)
    v, f = meshes[name + "_v"], meshes[name + "_f"]
    verts = batch_verts(v, n, rng, 0.01)
    cams = make_cams(n, rng, extent=float(np.abs(v).max()))
    ndc = O.to_ndc(O.project(verts, cams), flip_y=True)
    ndc[..., 0] += shift
    ndc[..., 2] += 2.732   # view depth of the reference's camera (App-A.1)
    return ndc.astype(np.float32), np.ascontiguousarray(f)


def _frags(ndc, f, H, K, blur, clip, grad=False):
    from acfm_video_3d_reconstruction_amd import ops
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.renderer import Fragments
    d = _dev()
    tv = torch.tensor(ndc, device=d, requires_grad=grad)
    return tv, Fragments(*ops.rasterize_fragments(tv, torch.from_numpy(f).to(d), H, K, blur_radius=blur,
                                                  clip_barycentric_coords=clip))


def _close(got, ref, floor=1e-9, what="", rel_l2=1e-5):
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    scale = float(ref.abs().max())
    err = float((got - ref).abs().max())
    print("%s: scale %.3g, max err %.3g" % (what, scale, err))
    assert err <= 1e-4 * scale + floor, what
    if scale > 1e3 * floor:
        rel = float((got - ref).norm() / ref.norm())
        assert rel <= rel_l2, (what, rel)


def _img(got, ref, what=""):
    err = float((got.detach().double().cpu() - ref.detach().double().cpu()).abs().max())
    print("%s: max err %.3g" % (what, err))
    assert err <= 1e-6, what


def _leaf(t):
    return t.detach().double().cpu().requires_grad_(True)


# ---- float64 restatements (App-A.5, A.6, A.10)
def _ref_alpha(p2f, dists, sigma):
    prob = torch.sigmoid(-dists / sigma) * (p2f >= 0)
    return prob, 1.0 - torch.prod(1.0 - prob, dim=-1)


def _ref_softmax(p2f, dists, zbuf, colors, sigma, gamma, bg, znear=1.0, zfar=100.0):
    mask = (p2f >= 0).double()
    prob, alpha = _ref_alpha(p2f, dists, sigma)
    z_inv = (zfar - zbuf) / (zfar - znear) * mask
    z_max = torch.max(z_inv, dim=-1).values[..., None].clamp(min=EPS)
    w = prob * torch.exp((z_inv - z_max) / gamma)
    delta = torch.exp((EPS - z_max) / gamma).clamp(min=EPS)
    denom = w.sum(dim=-1)[..., None] + delta
    rgb = ((w[..., None] * colors).sum(dim=-2) + delta * torch.as_tensor(bg, dtype=torch.float64)) / denom
    return torch.cat([rgb, alpha[..., None]], dim=-1)


def _ref_interp(p2f, bary, attrs):
    vals = attrs[p2f.clamp(min=0)]                              # [..., K, 3, D]
    return (bary[..., None] * vals).sum(dim=-2) * (p2f >= 0)[..., None]


def _texel_index(p2f, bary, R):
    """TexturesAtlas.sample_textures' texel choice from the kernel's float32 barycentrics (oracle_atlas_shade)."""
    w01 = torch.where((p2f < 0)[..., None], torch.zeros_like(bary[..., :2]), bary[..., :2]).float()
    wxy = (w01 * R).to(torch.int64)
    below = (w01.sum(dim=-1) * R - wxy.float().sum(dim=-1)) <= 1.0
    wxy = torch.where(below[..., None], wxy, R - 1 - wxy).clamp(0, R - 1)
    return (p2f.clamp(min=0) * R + wxy[..., 1]) * R + wxy[..., 0]


# ---- 1. blends and interpolation vs float64
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("blur", [0.0, SIL_BLUR])
@pytest.mark.parametrize("K", [1, 8, 20])
@pytest.mark.parametrize("name,seed", [("bird", 1), ("horse", 2)])
def test_blends_vs_float64(meshes, name, seed, K, blur, clip):
    from acfm_video_3d_reconstruction_amd import ops
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.renderer import BlendParams
    d = _dev()
    N, H = 2, 64
    ndc, f = _scene(meshes, name, N, seed)
    _, fr = _frags(ndc, f, H, K, blur, clip)
    p2f = fr.pix_to_face.cpu()
    assert (p2f[..., 0] >= 0).float().mean() > 0.05
    g = torch.Generator().manual_seed(seed)
    G = torch.randn(N, H, H, 4, generator=g)
    # sigmoid_alpha_blend (silhouette: no colours; and with colours)
    for with_colors in (False, True):
        dists = fr.dists.detach().clone().requires_grad_(True)
        col = torch.rand(N, H, H, K, 3, generator=g).to(d).requires_grad_(True) if with_colors else None
        fr1 = fr._replace(dists=dists)
        out = ops.sigmoid_alpha_blend(col, fr1, BlendParams(1e-4, 1e-4, 0))
        (out * G.to(d)).sum().backward()
        rd = _leaf(dists)
        _, alpha = _ref_alpha(p2f, rd, 1e-4)
        rc = _leaf(col) if with_colors else None
        rgb = rc[..., 0, :] if with_colors else torch.ones(N, H, H, 3, dtype=torch.float64)
        ref = torch.cat([rgb, alpha[..., None]], -1)
        _img(out, ref, what="sigmoid image")
        (ref * G.double()).sum().backward()
        _close(dists.grad, rd.grad, what="sigmoid grad dists")
        if with_colors:
            _close(col.grad, rc.grad, what="sigmoid grad colours")
    # softmax_rgb_blend, dense colours
    for gamma in (1e-4, 1e-2):
        for bg in (0.0, (0.2, 0.5, 0.9)):
            dists = fr.dists.detach().clone().requires_grad_(True)
            zbuf = fr.zbuf.detach().clone().requires_grad_(True)
            col = torch.rand(N, H, H, K, 3, generator=g).to(d).requires_grad_(True)
            out = ops.softmax_rgb_blend(col, fr._replace(dists=dists, zbuf=zbuf), BlendParams(1e-4, gamma, bg))
            (out * G.to(d)).sum().backward()
            rd, rz, rc = _leaf(dists), _leaf(zbuf), _leaf(col)
            ref = _ref_softmax(p2f, rd, rz, rc, 1e-4, gamma, bg)
            tag = "softmax gamma=%g bg=%s" % (gamma, bg)
            _img(out, ref, what=tag + " image")
            (ref * G.double()).sum().backward()
            _close(dists.grad, rd.grad, what=tag + " grad dists")
            _close(zbuf.grad, rz.grad, what=tag + " grad zbuf")
            _close(col.grad, rc.grad, what=tag + " grad colours")
    # interpolate_face_attributes
    Fp, D = N * f.shape[0], 5
    attrs = torch.randn(Fp, 3, D, generator=g).to(d).requires_grad_(True)
    bary = fr.bary_coords.detach().clone().requires_grad_(True)
    out = ops.interpolate_face_attributes(fr.pix_to_face, bary, attrs)
    Gi = torch.randn(out.shape, generator=g)
    (out * Gi.to(d)).sum().backward()
    rb, ra = _leaf(bary), _leaf(attrs)
    ref = _ref_interp(p2f, rb, ra)
    # unclipped barycentrics with blur reach |b| >> 1 on thin faces: the three products cancel, so the float32 bar is
    # set by their magnitudes, sum_i |b_i a_i| (the kernel's error is a few ulp of it)
    bound = _ref_interp(p2f, rb.detach().abs(), ra.detach().abs())
    err = (out.detach().double().cpu() - ref.detach()).abs()
    assert bool((err <= 1e-6 * bound + 1e-7).all()), float((err - 1e-6 * bound).max())
    (ref * Gi.double()).sum().backward()
    _close(bary.grad, rb.grad, what="interp grad bary")
    _close(attrs.grad, ra.grad, what="interp grad attrs")


# ---- 2. / 3. the reference's compositions vs the fused renders
def _nr_inputs(meshes, n, seed):
    rng = np.random.default_rng(seed)
    v, f = meshes["bird_v"], meshes["bird_f"]
    verts = batch_verts(v, n, rng, 0.01)
    cams = make_cams(n, rng, extent=float(np.abs(v).max()))
    d = _dev()
    return torch.tensor(verts, device=d), torch.from_numpy(np.ascontiguousarray(f)).to(d), torch.tensor(cams, device=d)


def _reference_view(verts, cams):
    """nmr.py:143-149: project, flip y, look_at_view_transform(eye=(0,0,-2.732)) with R[0,0] *= -1."""
    from acfm_video_3d_reconstruction_amd import ops
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.renderer import look_at_view_transform
    d = verts.device
    vs = ops.project(verts, cams) * torch.tensor([1.0, -1.0, 1.0], device=d)
    R, T = look_at_view_transform(eye=((0, 0, -2.732),), device=d)
    R[:, 0, 0] *= -1
    return vs, R.to(d), T.to(d)


def test_reference_silhouette_composition(meshes):
    from acfm_video_3d_reconstruction_amd import ops
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.renderer import (BlendParams, MeshRasterizer, MeshRenderer,
                                                                          RasterizationSettings,
                                                                          SfMOrthographicCameras, SoftSilhouetteShader)
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.structures import Meshes
    d = _dev()
    H, n = 96, 3
    verts, f, cams = _nr_inputs(meshes, n, 61)
    faces = f[None].expand(n, -1, -1)
    G = torch.rand(n, H, H, device=d)
    v1 = verts.clone().requires_grad_(True)
    mask_ref, _ = ops.sil_render(v1, f, cams, H)
    (mask_ref * G).sum().backward()
    v2 = verts.clone().requires_grad_(True)
    vs, R, T = _reference_view(v2, cams)
    renderer = MeshRenderer(
        rasterizer=MeshRasterizer(cameras=SfMOrthographicCameras(device=d),
                                  raster_settings=RasterizationSettings(image_size=H, blur_radius=SIL_BLUR,
                                                                        faces_per_pixel=20, bin_size=None)),
        shader=SoftSilhouetteShader(blend_params=BlendParams(sigma=1e-4, gamma=1e-4, background_color=0)))
    img = renderer(meshes_world=Meshes(verts=vs, faces=faces), R=R, T=T)
    assert img.shape == (n, H, H, 4) and bool((img[..., :3] == 1).all())
    alpha = img[..., 3]
    assert float((alpha - mask_ref).abs().max()) <= 1e-6
    mask_o, _ = O.sil_render(verts.cpu().numpy(), f.cpu().numpy(), cams.cpu().numpy(), H)
    assert float(np.abs(alpha.detach().cpu().numpy() - mask_o).max()) <= 1e-6
    (alpha * G).sum().backward()
    _close(v2.grad, v1.grad, floor=0.0, what="silhouette vertex gradient")


def _tex_renderer(d, H, K, blur, clip, gamma, lights=None):
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.renderer import (BlendParams, DirectionalLights,
                                                                          MeshRasterizer, MeshRenderer,
                                                                          RasterizationSettings,
                                                                          SfMOrthographicCameras, SoftPhongShader)
    cameras = SfMOrthographicCameras(device=d)
    lights = lights or DirectionalLights(ambient_color=((1., 1., 1.),), diffuse_color=((0., 0., 0.),),
                                         specular_color=((0., 0., 0.),), direction=((0., 1., 0.),))
    return MeshRenderer(
        rasterizer=MeshRasterizer(cameras=cameras, raster_settings=RasterizationSettings(
            image_size=H, blur_radius=blur, faces_per_pixel=K, clip_barycentric_coords=clip)),
        shader=SoftPhongShader(device=d, cameras=cameras, lights=lights.clone().to(d),
                               blend_params=BlendParams(1e-4, gamma, background_color=0)))


def test_reference_texture_composition(meshes):
    from acfm_video_3d_reconstruction_amd import ops
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.renderer import TexturesAtlas
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.structures import Meshes
    d = _dev()
    H, n, R = 96, 3, 6
    verts, f, cams = _nr_inputs(meshes, n, 62)
    atlas = torch.rand(n, f.shape[0], R, R, 3, device=d)
    G = torch.rand(n, 3, H, H, device=d)
    a1 = atlas.clone().requires_grad_(True)
    imgs_ref, sil_ref, _ = ops.tex_render(verts, f, cams, a1, H)
    (imgs_ref * G).sum().backward()
    a2 = atlas.clone().requires_grad_(True)
    vs, Rm, T = _reference_view(verts, cams)
    mesh = Meshes(verts=vs, faces=f[None].expand(n, -1, -1), textures=TexturesAtlas(atlas=a2))
    img = _tex_renderer(d, H, 1, 0.0, True, 1e-4)(meshes_world=mesh, R=Rm, T=T)
    rgb = img[..., :3].permute(0, 3, 1, 2)
    assert float((rgb - imgs_ref).abs().max()) <= 1e-6
    assert float((img[..., 3] - sil_ref).abs().max()) <= 1e-6
    imgs_o, sil_o, _, _ = O.tex_render(verts.cpu().numpy(), f.cpu().numpy(), cams.cpu().numpy(),
                                       atlas.cpu().numpy(), H)
    assert float(np.abs(rgb.detach().cpu().numpy() - imgs_o).max()) <= 1e-6
    assert float(np.abs(img[..., 3].detach().cpu().numpy() - sil_o).max()) <= 1e-6
    (rgb * G).sum().backward()
    _close(a2.grad, a1.grad, floor=0.0, what="atlas gradient")


# ---- 4. soft textured render
@pytest.mark.parametrize("K", [8, 20])
def test_soft_textured_render(meshes, K):
    from acfm_video_3d_reconstruction_amd import ops
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.renderer import BlendParams
    d = _dev()
    N, H, R, gamma = 2, 64, 4, 1e-2
    ndc, f = _scene(meshes, "bird", N, 70 + K)
    tv, fr = _frags(ndc, f, H, K, SIL_BLUR, False, grad=True)
    g = torch.Generator().manual_seed(K)
    atlas = torch.rand(N * f.shape[0], R, R, 3, generator=g).to(d).requires_grad_(True)
    amb = torch.tensor([[0.9, 1.0, 0.8]], device=d)
    bp = BlendParams(1e-4, gamma, (0.1, 0.2, 0.3))
    img = ops.atlas_softmax_blend(atlas, fr, bp, ambient=amb)
    G = torch.randn(N, H, H, 4, generator=g)
    (img * G.to(d)).sum().backward()
    p2f = fr.pix_to_face.cpu()
    rd, rz, ra = _leaf(fr.dists), _leaf(fr.zbuf), _leaf(atlas)
    ti = _texel_index(p2f, fr.bary_coords.detach().cpu(), R)
    colors = ra.reshape(-1, 3)[ti] * amb.cpu().double()
    ref = _ref_softmax(p2f, rd, rz, colors, 1e-4, gamma, (0.1, 0.2, 0.3))
    _img(img, ref, what="soft textured image")
    (ref * G.double()).sum().backward()
    _close(atlas.grad, ra.grad, what="soft textured atlas gradient")
    # the vertex gradient: the rasterizer's (oracle-pinned) backward fed with the restatement's fragment gradients
    tv2, fr2 = _frags(ndc, f, H, K, SIL_BLUR, False, grad=True)
    ((fr2.dists * rd.grad.float().to(d)).sum() + (fr2.zbuf * rz.grad.float().to(d)).sum()).backward()
    _close(tv.grad, tv2.grad, floor=0.0, what="soft textured vertex gradient")


# ---- 5. vertex colours, 6. Phong
def test_vertex_colours_send_gradients(meshes):
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.renderer import Textures
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.structures import Meshes
    d = _dev()
    H, n = 64, 2
    verts, f, cams = _nr_inputs(meshes, n, 63)
    v = verts.clone().requires_grad_(True)
    rgb = torch.rand(n, verts.shape[1], 3, device=d, requires_grad=True)
    vs, Rm, T = _reference_view(v, cams)
    mesh = Meshes(verts=vs, faces=f[None].expand(n, -1, -1), textures=Textures(verts_rgb=rgb))
    img = _tex_renderer(d, H, 8, SIL_BLUR, False, 1e-2)(meshes_world=mesh, R=Rm, T=T)
    (img * torch.rand_like(img)).sum().backward()
    for t in (v.grad, rgb.grad):
        assert t is not None and bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0


def _ref_phong(verts, faces, p2f, bary, texels, light, spec_color, diff_color, amb, cam_center, shininess, point):
    """float64 restatement of phong_shading (App-A.10): interpolated positions and vertex normals, relu(n.l) diffuse,
    relu(v.r)^s [n.l > 0] specular, (ambient + diffuse) texels + specular."""
    import torch.nn.functional as Fn
    fv = verts[faces]
    n = torch.zeros_like(verts)
    for a, b, c in ((1, 2, 0), (2, 0, 1), (0, 1, 2)):
        n = n.index_add(0, faces[:, a], torch.cross(fv[:, b] - fv[:, a], fv[:, c] - fv[:, a], dim=1))
    n = Fn.normalize(n, eps=1e-6, dim=1)
    pts = _ref_interp(p2f, bary, fv)
    nrm = Fn.normalize(_ref_interp(p2f, bary, n[faces]), eps=1e-6, dim=-1)
    sh = (-1,) + (1,) * (pts.dim() - 2) + (3,)
    l = Fn.normalize(light.reshape(sh) - pts if point else light.reshape(sh).expand_as(pts), eps=1e-6, dim=-1)
    cos = (nrm * l).sum(-1)
    diffuse = diff_color * torch.relu(cos)[..., None]
    view = Fn.normalize(cam_center.reshape(sh) - pts, eps=1e-6, dim=-1)
    refl = -l + 2 * cos[..., None] * nrm
    spec = spec_color * (torch.relu((view * refl).sum(-1)) * (cos > 0)).pow(shininess)[..., None]
    return (amb + diffuse) * texels + spec


def _camera_centre(R, T):
    """World position of a camera whose view is X R + T: C R + T = 0, C = -T R^T for a rotation R."""
    return -(T.double()[:, None, :] @ R.double().transpose(1, 2))[:, 0]


@pytest.mark.parametrize("point", [False, True])
def test_phong_shading_vs_float64(meshes, point):
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.renderer import (DirectionalLights, Materials, PointLights,
                                                                          SfMOrthographicCameras)
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.renderer.mesh.shading import phong_shading
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.structures import Meshes
    d = _dev()
    N, H, K = 2, 64, 8
    ndc, f = _scene(meshes, "horse", N, 80 + point)
    _, fr = _frags(ndc, f, H, K, SIL_BLUR, True)
    fr = fr._replace(**{k: getattr(fr, k).detach() for k in ("zbuf", "bary_coords", "dists")})
    kw = dict(ambient_color=((0.3, 0.3, 0.3),), diffuse_color=((0.6, 0.5, 0.4),), specular_color=((0.5, 0.5, 0.5),))
    lights = PointLights(location=((0.5, 1.0, -2.0),), device=d, **kw) if point else \
        DirectionalLights(direction=((0.3, 1.0, -1.0),), device=d, **kw)
    cam = SfMOrthographicCameras(device=d, T=torch.tensor([[0.0, 0.0, 2.732]]))
    v = torch.tensor(ndc, device=d, requires_grad=True)
    faces = torch.from_numpy(f).to(d)[None].expand(N, -1, -1)
    mesh = Meshes(verts=v, faces=faces)
    texels = torch.rand(N, H, H, K, 3, device=d, requires_grad=True)
    col = phong_shading(mesh, fr, lights, cam, Materials(device=d, shininess=64), texels)
    G = torch.randn_like(col)
    (col * G).sum().backward()
    rv, rt = _leaf(v), _leaf(texels)
    loc = lights.location if point else lights.direction
    ref = _ref_phong(rv.reshape(-1, 3), mesh.faces_packed().cpu(), fr.pix_to_face.cpu(), fr.bary_coords.cpu().double(),
                     rt, loc.cpu().double(), 0.5, torch.tensor([0.6, 0.5, 0.4], dtype=torch.float64), 0.3,
                     _camera_centre(torch.eye(3)[None], torch.tensor([[0.0, 0.0, 2.732]])), 64, point)
    # the lighting terms are float32 torch: relu(v.r)^64 multiplies their rounding by 64, so the colours take the
    # gradient bars here (1e-4 of scale, 1e-5 relative L2), not the 1e-6 of a blend
    _close(col, ref, floor=0.0, what="phong colours")
    (ref * G.cpu().double()).sum().backward()
    _close(texels.grad, rt.grad, what="phong grad texels")
    # the vertex gradient runs back through the same float32 lighting (pow 64 of relu(v.r), two normalisations):
    # measured 1.2e-5 relative L2 for the point light; the max-error bar stays 1e-4 of scale
    _close(v.grad, rv.grad, floor=1e-6, what="phong grad verts", rel_l2=2e-5)


# ---- 7. determinism, 8. hipGraph, 9. edge cases
def test_scattering_backwards_deterministic(meshes):
    from acfm_video_3d_reconstruction_amd import _lib, ops
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.renderer import BlendParams
    d = _dev()
    N, H, K, R = 3, 96, 8, 6
    ndc, f = _scene(meshes, "cow", N, 90)
    _, fr = _frags(ndc, f, H, K, SIL_BLUR, True)
    atlas = torch.rand(N * f.shape[0], R, R, 3, device=d)
    attrs = torch.randn(N * f.shape[0], 3, 4, device=d)
    G, Gi = torch.randn(N, H, H, 4, device=d), torch.randn(N, H, H, K, 4, device=d)

    def grads():
        a, fa = atlas.clone().requires_grad_(True), attrs.clone().requires_grad_(True)
        img = ops.atlas_softmax_blend(a, fr, BlendParams(1e-4, 1e-2, 0))
        out = ops.interpolate_face_attributes(fr.pix_to_face, fr.bary_coords, fa)
        return torch.autograd.grad((img * G).sum() + (out * Gi).sum(), [a, fa])

    with _lib.raster_tuning(deterministic=True):
        x, y = grads(), grads()
    z = grads()
    for a, b, c in zip(x, y, z):
        assert float(a.abs().max()) > 0 and torch.equal(a, b)
        assert float((a - c).abs().max()) <= 1e-6 * float(c.abs().max())


def test_silhouette_shader_graph_capture(meshes):
    from acfm_video_3d_reconstruction_amd import ops
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.renderer import BlendParams, Fragments, SoftSilhouetteShader
    d = _dev()
    ndc, f = _scene(meshes, "bird", 2, 91)
    H, K = 64, 20
    tv = torch.tensor(ndc, device=d, requires_grad=True)
    faces = torch.from_numpy(f).to(d)
    G = torch.rand(2, H, H, device=d)
    shader = SoftSilhouetteShader(BlendParams(1e-4, 1e-4, 0))

    def step():
        fr = Fragments(*ops.rasterize_fragments(tv, faces, H, K, blur_radius=SIL_BLUR))
        alpha = shader(fr, None)[..., 3]
        (gv,) = torch.autograd.grad((alpha * G).sum(), [tv])
        return alpha, gv

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = step()
    for _ in range(2):
        ops.graph_replay(g)
    torch.cuda.synchronize()
    got = [t.detach().clone() for t in outs]
    ref = [t.detach() for t in step()]
    assert torch.equal(got[0], ref[0])
    assert float((got[1] - ref[1]).abs().max()) <= 1e-5 * float(ref[1].abs().max())


def test_mesh_off_screen_and_constant_verts(meshes):
    from acfm_video_3d_reconstruction_amd import ops
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.renderer import BlendParams
    d = _dev()
    N, H, K = 2, 32, 8
    ndc, f = _scene(meshes, "bird", N, 92, shift=10.0)
    tv, fr = _frags(ndc, f, H, K, SIL_BLUR, False, grad=True)
    assert bool((fr.pix_to_face < 0).all())
    atlas = torch.rand(N * f.shape[0], 4, 4, 3, device=d, requires_grad=True)
    img = ops.atlas_softmax_blend(atlas, fr, BlendParams(1e-4, 1e-4, (0.1, 0.2, 0.3)))
    assert torch.allclose(img[..., :3], torch.tensor([0.1, 0.2, 0.3], device=d).expand(N, H, H, 3), atol=1e-6)
    assert bool((img[..., 3] == 0).all())
    sil = ops.sigmoid_alpha_blend(None, fr, BlendParams())
    ((img * torch.rand_like(img)).sum() + sil.sum()).backward()
    for t in (tv.grad, atlas.grad):
        assert bool(torch.isfinite(t).all()) and float(t.abs().max()) == 0.0
    # vertices that do not require grad: no vertex gradient is formed, the atlas still gets one
    ndc, f = _scene(meshes, "bird", N, 93)
    tv, fr = _frags(ndc, f, H, K, SIL_BLUR, False, grad=False)
    atlas = torch.rand(N * f.shape[0], 4, 4, 3, device=d, requires_grad=True)
    ops.atlas_softmax_blend(atlas, fr, BlendParams(1e-4, 1e-2, 0)).sum().backward()
    assert tv.grad is None and not fr.dists.requires_grad
    assert float(atlas.grad.abs().max()) > 0


# ---- the Phong shaders end to end (diffuse and specular light: phong_shading + the dense blends)
def _vertex_colour_scene(meshes, n, seed):
    d = _dev()
    verts, f, cams = _nr_inputs(meshes, n, seed)
    vs, Rm, T = _reference_view(verts, cams)
    rgb = torch.rand(n, verts.shape[1], 3, device=d, generator=torch.Generator(device=d).manual_seed(seed))
    return vs.detach(), f, Rm, T, rgb


def _phong_lights(d):
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.renderer import DirectionalLights
    return DirectionalLights(ambient_color=((0.3, 0.3, 0.3),), diffuse_color=((0.6, 0.5, 0.4),),
                             specular_color=((0.5, 0.5, 0.5),), direction=((0.3, 1.0, -1.0),), device=d)


def _ref_shaded(vs, f, fr, rgb, Rm, T):
    """float64 texels (vertex colours interpolated) and Phong colours of _phong_lights, at the kernel's fragments."""
    n = vs.shape[0]
    V = vs.shape[1]
    faces = (f.cpu()[None] + V * torch.arange(n)[:, None, None]).reshape(-1, 3)
    p2f, bary = fr.pix_to_face.cpu(), fr.bary_coords.detach().cpu().double()
    texels = _ref_interp(p2f, bary, rgb.reshape(-1, 3)[faces])
    cols = _ref_phong(vs.detach().cpu().double().reshape(-1, 3), faces, p2f, bary, texels,
                      torch.tensor([[0.3, 1.0, -1.0]], dtype=torch.float64), 0.5,
                      torch.tensor([0.6, 0.5, 0.4], dtype=torch.float64), 0.3, _camera_centre(Rm.cpu(), T.cpu()), 64,
                      False)
    return cols


def test_soft_phong_shader_with_diffuse_and_specular(meshes):
    """SoftPhongShader with diffuse and specular light over vertex colours (phong_shading and the dense softmax
    kernel) against the float64 restatement; the image takes the gradient bars (float32 lighting, pow 64), the
    colour gradient the usual ones."""
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.renderer import Textures
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.structures import Meshes
    d = _dev()
    n, H, K, gamma = 2, 64, 8, 1e-2
    vs, f, Rm, T, rgb = _vertex_colour_scene(meshes, n, 101)
    rgb = rgb.requires_grad_(True)
    renderer = _tex_renderer(d, H, K, SIL_BLUR, True, gamma, lights=_phong_lights(d))
    mesh = Meshes(verts=vs, faces=f[None].expand(n, -1, -1), textures=Textures(verts_rgb=rgb))
    img = renderer(meshes_world=mesh, R=Rm, T=T)
    G = torch.randn_like(img)
    (img * G).sum().backward()
    fr = renderer.rasterizer(mesh, R=Rm, T=T)
    rr = _leaf(rgb)
    cols = _ref_shaded(vs, f, fr, rr, Rm, T)
    ref = _ref_softmax(fr.pix_to_face.cpu(), fr.dists.detach().cpu().double(), fr.zbuf.detach().cpu().double(), cols,
                       1e-4, gamma, 0.0)
    assert float(ref[..., 3].max()) > 0.5
    _close(img, ref, floor=0.0, what="soft phong image")
    (ref * G.cpu().double()).sum().backward()
    _close(rgb.grad, rr.grad, what="soft phong grad verts_rgb")


def test_hard_phong_shader(meshes):
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.renderer import (BlendParams, HardPhongShader,
                                                                          MeshRasterizer, MeshRenderer,
                                                                          RasterizationSettings,
                                                                          SfMOrthographicCameras, Textures)
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.structures import Meshes
    d = _dev()
    n, H = 2, 64
    vs, f, Rm, T, rgb = _vertex_colour_scene(meshes, n, 102)
    cameras = SfMOrthographicCameras(device=d)
    renderer = MeshRenderer(
        rasterizer=MeshRasterizer(cameras=cameras, raster_settings=RasterizationSettings(
            image_size=H, faces_per_pixel=1, clip_barycentric_coords=True)),
        shader=HardPhongShader(device=d, cameras=cameras, lights=_phong_lights(d),
                               blend_params=BlendParams(background_color=(0.1, 0.2, 0.3))))
    mesh = Meshes(verts=vs, faces=f[None].expand(n, -1, -1), textures=Textures(verts_rgb=rgb))
    img = renderer(meshes_world=mesh, R=Rm, T=T)
    fr = renderer.rasterizer(mesh, R=Rm, T=T)
    cols = _ref_shaded(vs, f, fr, rgb.cpu().double(), Rm, T)
    empty = (fr.pix_to_face.cpu()[..., 0] < 0)[..., None]
    ref_rgb = torch.where(empty, torch.tensor([0.1, 0.2, 0.3], dtype=torch.float64), cols[..., 0, :])
    assert 0.05 < float((~empty).double().mean()) < 0.95
    _close(img[..., :3], ref_rgb, floor=0.0, what="hard phong image")
    assert bool((img[..., 3] == 1).all())


def test_shader_entry_points_refuse_half_storage(meshes):
    """Tuning flags bit 1 (half storage) is refused by every shader entry point (ACFM_E_BADARG); the same calls with
    the plain tuning run."""
    import ctypes
    from acfm_video_3d_reconstruction_amd import _lib, ops
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.renderer import BlendParams
    d = _dev()
    ndc, f = _scene(meshes, "bird", 1, 103)
    _, fr = _frags(ndc, f, 32, 8, SIL_BLUR, False)
    K, P = 8, 32 * 32
    Fp, R = f.shape[0], 4
    p2f, zb, by, ds = (t.detach().contiguous() for t in fr)
    cols = torch.rand(P, K, 3, device=d)
    atlas = torch.rand(Fp, R, R, 3, device=d)
    attrs = torch.rand(Fp, 3, 2, device=d)
    rgba = torch.empty(P, 4, device=d)
    g = torch.rand(P, 4, device=d)
    gd, gz, gc = torch.empty(P, K, device=d), torch.empty(P, K, device=d), torch.empty(P, K, 3, device=d)
    gb, gf = torch.empty(P, K, 3, device=d), torch.empty_like(attrs)
    out = torch.empty(P, K, 2, device=d)
    gout = torch.rand(P, K, 2, device=d)
    bp = ops.blend_struct(BlendParams(1e-4, 1e-2, 0))
    q = _lib.ptr
    calls = {
        "acfm_sigmoid_alpha_blend": lambda t: (q(p2f), q(ds), None, P, K, 1e-4, q(rgba), t),
        "acfm_sigmoid_alpha_blend_backward": lambda t: (q(p2f), q(ds), q(g), P, K, 1e-4, q(gd), q(gc), t),
        "acfm_softmax_rgb_blend": lambda t: (q(p2f), q(ds), q(zb), q(by), None, q(atlas), R, Fp, None, P, K, P,
                                             ctypes.byref(bp), q(rgba), t),
        "acfm_softmax_rgb_blend_backward": lambda t: (q(p2f), q(ds), q(zb), q(by), q(cols), None, 0, 0, None, P, K, P,
                                                      ctypes.byref(bp), q(g), q(gd), q(gz), q(gc), None, None, 0, t),
        "acfm_interpolate_face_attributes": lambda t: (q(p2f), q(by), q(attrs), P, K, Fp, 2, q(out), t),
        "acfm_interpolate_face_attributes_backward": lambda t: (q(p2f), q(by), q(attrs), q(gout), P, K, Fp, 2, q(gb),
                                                                q(gf), None, 0, t),
    }
    f16 = _lib.with_f16(None, True)
    for name, args in calls.items():
        with pytest.raises(RuntimeError, match="ACFM_E_BADARG"):
            _lib.call(name, d, *args(_lib.tuning_ptr(f16)))
        _lib.call(name, d, *args(None))
    torch.cuda.synchronize()
