"""GPU: TexturesUV.sample_textures on the HIP kernel (ops.uv_texels) against the float64 composition on
the kernel's own float32 inputs.  Bars: texels 1e-5 absolute for maps in [0,1] (three float32 roundings of a
coordinate of at most 6 texels are about 1e-6; torch's own float32 grid_sample stays within 8.1e-7 of float64 on these
shapes), rendered images 1e-6, gradients the shader tests' rule (1e-4 of their scale + 1e-9, 1e-5 relative L2).

The derivative with respect to uv jumps where a sampling coordinate crosses an integer, so slots whose float64
coordinate lies within 1e-5 texel of one are left out of the grad_bary / grad_faces_verts_uvs comparisons (their
upstream gradient is zeroed for that run); the slots placed at uv = 0, 1 and a texel centre on purpose are among
them, and at most 1 % of the others may be.  The forward and grad_maps are continuous there and see every slot."""
import functools
import math

import pytest
import torch

import uv_reference as U
from test_gpu_shaders import (SIL_BLUR, _camera_centre, _close, _dev, _img, _nr_inputs, _ref_phong,  # noqa: F401
                              _reference_view)

pytestmark = pytest.mark.gpu

N, H, W, F, HM, WM = 2, 9, 9, 6, 5, 7     # 81 pixels a mesh: the last block is partial; an odd, non-square map


@functools.lru_cache(maxsize=None)
def _case(K, align_corners, padding_mode):
    """Hand-built fragments (float32, host) and their float64 reference, computed once per parameter set."""
    g = torch.Generator().manual_seed(1000 + 10 * K + 2 * int(align_corners) + (padding_mode == "zeros"))
    p2f = torch.randint(-1, F, (N, H, W, K), generator=g)
    bary = torch.rand(N, H, W, K, 3, generator=g) + 0.05
    bary = bary / bary.sum(dim=-1, keepdim=True)
    fv = torch.rand(N * F, 3, 2, generator=g) * 1.4 - 0.2            # [-0.2, 1.2]: taps fall outside the map
    special = torch.zeros(N, H, W, K, dtype=torch.bool)
    for n in range(N):                                               # uv exactly 0, 1 and a texel centre (3, 2)
        for j, uv in enumerate(((0.0, 0.0), (1.0, 1.0), (0.5, 0.5))):
            p2f[n, 2 + j, 3 + n, 0] = j
            bary[n, 2 + j, 3 + n, 0] = torch.tensor([1.0, 0.0, 0.0])
            fv[n * F + j, 0] = torch.tensor(uv)
            special[n, 2 + j, 3 + n, 0] = True
    p2f = torch.where(p2f >= 0, p2f + F * torch.arange(N).reshape(N, 1, 1, 1), p2f)
    maps = torch.rand(N, HM, WM, 3, generator=g)
    G = torch.randn(N, H, W, K, 3, generator=g)
    # slots near an integer coordinate (the unclamped one: border padding clamps at integers too)
    x, y = U.coords(p2f, bary.double(), fv.double(), HM, WM, align_corners, "zeros")
    live = p2f >= 0
    near = live & (((x - x.round()).abs() <= 1e-5) | ((y - y.round()).abs() <= 1e-5))
    others = live & ~special
    left_out = float((near & others).sum()) / float(others.sum())
    keep = ~(near | special)

    def ref(Gk):
        rb, rf, rm = (t.double().requires_grad_(True) for t in (bary, fv, maps))
        out = U.composition(p2f, rb, rf, rm, align_corners, padding_mode)
        (out * Gk.double()).sum().backward()
        return out.detach(), rb.grad, rf.grad, rm.grad

    Gk = G * keep[..., None]
    return dict(p2f=p2f, bary=bary, fv=fv, maps=maps, G=G, Gk=Gk, keep=keep, left_out=left_out, special=special,
                ref_all=ref(G), ref_keep=ref(Gk))


def _run(c, Gname, align_corners, padding_mode):
    from acfm_video_3d_reconstruction_amd import ops
    d = _dev()
    b, fv, m = (c[k].to(d).requires_grad_(True) for k in ("bary", "fv", "maps"))
    out = ops.uv_texels(c["p2f"].to(d), b, fv, m, align_corners=align_corners, padding_mode=padding_mode)
    (out * c[Gname].to(d)).sum().backward()
    return out, b.grad, fv.grad, m.grad


# ---- 1. hand-built fragments vs float64
@pytest.mark.parametrize("padding_mode", ["border", "zeros"])
@pytest.mark.parametrize("align_corners", [True, False])
@pytest.mark.parametrize("K", [1, 4])
def test_uv_texels_vs_float64(K, align_corners, padding_mode):
    c = _case(K, align_corners, padding_mode)
    print("left out %.4f of the ordinary slots" % c["left_out"])
    assert c["left_out"] <= 0.01
    out, _, _, gm = _run(c, "G", align_corners, padding_mode)
    r_out, _, _, r_gm = c["ref_all"]
    err = float((out.detach().double().cpu() - r_out).abs().max())
    print("texels: max err %.3g" % err)
    assert tuple(out.shape) == (N, H, W, K, 3) and err <= 1e-5
    _close(gm, r_gm, what="grad_maps")
    out, gb, gf, gm = _run(c, "Gk", align_corners, padding_mode)
    _, r_gb, r_gf, r_gm = c["ref_keep"]
    _close(gb, r_gb, what="grad_bary")
    _close(gf, r_gf, what="grad_faces_verts_uvs")
    _close(gm, r_gm, what="grad_maps (kept slots)")
    assert float(gb.cpu()[c["p2f"] < 0].abs().max()) == 0.0          # nothing reaches an empty slot's barycentrics


def test_empty_slots_sample_and_scatter_at_uv_zero():
    """Empty slots hold maps[n, Hm-1, 0] exactly (the defaults), and a gradient sent into them lands there."""
    from acfm_video_3d_reconstruction_amd import ops
    d = _dev()
    c = _case(4, True, "border")
    p2f = c["p2f"].to(d)
    empty = p2f < 0
    m = c["maps"].to(d).requires_grad_(True)
    out = ops.uv_texels(p2f, c["bary"].to(d), c["fv"].to(d), m)
    for n in range(N):
        assert torch.equal(out[n][empty[n]], m[n, HM - 1, 0].detach().expand(int(empty[n].sum()), 3))
    Ge = c["G"].to(d) * empty[..., None]
    (gm,) = torch.autograd.grad((out * Ge).sum(), [m])
    want = torch.zeros_like(gm)
    want[:, HM - 1, 0] = Ge.double().sum(dim=(1, 2, 3)).float()
    assert float(want.abs().min(dim=-1).values[:, HM - 1, 0].min()) > 0
    _close(gm, want, what="grad_maps from empty slots")
    assert float((gm - want).abs().sum()) == float((gm - want)[:, HM - 1, 0].abs().sum())   # no other texel touched


# ---- 2. through the renderer
class _FixedTexels:
    """A texture whose sample_textures returns the texels it was given (the reference feeds float64 texels)."""

    def __init__(self, texels):
        self.texels = texels

    def sample_textures(self, fragments, **kwargs):
        return self.texels


@pytest.mark.parametrize("shader,K,blur", [("soft", 4, SIL_BLUR), ("soft", 1, 0.0), ("hard", 1, 0.0)])
def test_uv_textures_through_the_renderer(meshes, shader, K, blur):
    from acfm_video_3d_reconstruction_amd import texture
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.renderer import (BlendParams, DirectionalLights,
                                                                          HardPhongShader, MeshRasterizer, MeshRenderer,
                                                                          RasterizationSettings,
                                                                          SfMOrthographicCameras, SoftPhongShader,
                                                                          TexturesUV)
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.structures import Meshes
    d = _dev()
    n, S = 2, 32
    verts, f, cams = _nr_inputs(meshes, n, 120 + K)
    uv0 = torch.tensor((texture.get_spherical_coords(meshes["bird_v"]) + 1.0) / 2.0, dtype=torch.float32, device=d)
    g = torch.Generator().manual_seed(K)
    maps0 = torch.rand(n, 16, 32, 3, generator=g).to(d)
    faces = f[None].expand(n, -1, -1)
    cameras = SfMOrthographicCameras(device=d)
    lights = DirectionalLights(ambient_color=((0.3, 0.3, 0.3),), diffuse_color=((0.6, 0.5, 0.4),),
                               specular_color=((0.0, 0.0, 0.0),), direction=((0.3, 1.0, -1.0),), device=d)
    bp = BlendParams(1e-4, 1e-2, (0.1, 0.2, 0.3))
    sh = (SoftPhongShader if shader == "soft" else HardPhongShader)(device=d, cameras=cameras, lights=lights,
                                                                   blend_params=bp)
    renderer = MeshRenderer(rasterizer=MeshRasterizer(cameras=cameras, raster_settings=RasterizationSettings(
        image_size=S, blur_radius=blur, faces_per_pixel=K, clip_barycentric_coords=True)), shader=sh)

    v1 = verts.clone().requires_grad_(True)
    maps1 = maps0.clone().requires_grad_(True)
    vu1 = uv0[None].expand(n, -1, -1).clone().requires_grad_(True)
    vs, Rm, T = _reference_view(v1, cams)
    mesh = Meshes(verts=vs, faces=faces, textures=TexturesUV(maps=maps1, faces_uvs=faces, verts_uvs=vu1))
    img = renderer(meshes_world=mesh, R=Rm, T=T)
    G = torch.randn(img.shape, generator=g).to(d)
    (img * G).sum().backward()
    assert 0.05 < float((renderer.rasterizer(mesh, R=Rm, T=T).pix_to_face[..., 0] >= 0).float().mean()) < 0.95

    # the same shader fed float64 texels of the composition on the same fragments
    v2 = verts.clone().requires_grad_(True)
    vs2, _, _ = _reference_view(v2, cams)
    mesh2 = Meshes(verts=vs2, faces=faces)
    fr = renderer.rasterizer(mesh2, R=Rm, T=T)
    p2f = fr.pix_to_face.cpu()
    rb, rm, rvu = (t.detach().double().cpu().requires_grad_(True) for t in (fr.bary_coords, maps0, vu1))
    V = rvu.shape[1]
    rfv = rvu.reshape(-1, 2)[(f.cpu()[None] + V * torch.arange(n)[:, None, None]).reshape(-1, 3)]
    t64 = U.composition(p2f, rb, rfv, rm)
    t32 = t64.detach().float().to(d).requires_grad_(True)
    mesh2.textures = _FixedTexels(t32)
    ref = sh(fr, mesh2, R=Rm, T=T)
    _img(img, ref, what="%s uv image" % shader)
    (gt,) = torch.autograd.grad((ref * G).sum(), [t32], retain_graph=True)
    (t64 * gt.double().cpu()).sum().backward()
    ((ref * G).sum() + (fr.bary_coords * rb.grad.float().to(d)).sum()).backward()
    _close(maps1.grad, rm.grad, what="%s uv grad maps" % shader)
    _close(vu1.grad, rvu.grad, what="%s uv grad verts_uvs" % shader)
    _close(v1.grad, v2.grad, floor=0.0, what="%s uv grad verts" % shader)


# ---- 3. deterministic mode
def test_uv_backward_deterministic():
    from acfm_video_3d_reconstruction_amd import _lib
    c = _case(4, False, "zeros")

    def grads():
        _, _, gf, gm = _run(c, "G", False, "zeros")
        return gm, gf

    with _lib.raster_tuning(deterministic=True):
        x, y = grads(), grads()
    z = grads()
    for a, b, r in zip(x, y, z):
        assert float(a.abs().max()) > 0 and torch.equal(a, b)
        assert float((a - r).abs().max()) <= 1e-6 * float(r.abs().max())
    _close(x[0], c["ref_all"][3], what="deterministic grad_maps")


# ---- 4. graph capture
def test_uv_texels_graph_capture():
    from acfm_video_3d_reconstruction_amd import ops
    d = _dev()
    c = _case(4, True, "border")
    p2f, G = c["p2f"].to(d), c["G"].to(d)
    b, fv, m = (c[k].to(d).requires_grad_(True) for k in ("bary", "fv", "maps"))

    def step():
        out = ops.uv_texels(p2f, b, fv, m)
        return (out,) + torch.autograd.grad((out * G).sum(), [b, fv, m])

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    with torch.no_grad():
        m.copy_(torch.rand(m.shape, generator=torch.Generator().manual_seed(5)).to(d))   # a new map, then replay
    for _ in range(2):
        ops.graph_replay(graph)
    torch.cuda.synchronize()
    got = [t.detach().clone() for t in outs]
    ref = [t.detach() for t in step()]
    assert not torch.equal(got[0], c["ref_all"][0].float().to(d))
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    for a, r in zip(got[2:], ref[2:]):
        assert float((a - r).abs().max()) <= 1e-5 * float(r.abs().max())


# ---- 5. no K-fold copy of the maps
def test_uv_texels_makes_no_k_fold_copy():
    from acfm_video_3d_reconstruction_amd import ops
    d = _dev()
    n, S, K, Fm, Hm = 2, 16, 8, 6, 256
    g = torch.Generator().manual_seed(6)
    p2f = torch.randint(-1, Fm, (n, S, S, K), generator=g)
    p2f = torch.where(p2f >= 0, p2f + Fm * torch.arange(n).reshape(n, 1, 1, 1), p2f).to(d)
    bary = torch.rand(n, S, S, K, 3, generator=g).to(d).requires_grad_(True)
    fv = torch.rand(n * Fm, 3, 2, generator=g).to(d).requires_grad_(True)
    maps = torch.rand(n, Hm, Hm, 3, generator=g).to(d).requires_grad_(True)
    G = torch.randn(n, S, S, K, 3, generator=g).to(d)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = ops.uv_texels(p2f, bary, fv, maps)
    grads = torch.autograd.grad((out * G).sum(), [bary, fv, maps])
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    k_fold = n * K * Hm * Hm * 3 * 4
    print("peak rise %.2f MB, one K-fold copy %.2f MB" % (rise / 1e6, k_fold / 1e6))
    assert float(grads[2].abs().max()) > 0
    assert rise < k_fold
