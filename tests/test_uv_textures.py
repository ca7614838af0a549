"""CPU: TexturesUV of the shim -- construction, the Textures(...) wrapper, refusals, and the host
sample_textures against a restatement with explicit floor and weights (no grid_sample: it pins the flip and the
x / y order); ops.uv_texels checks its shapes first and then refuses host tensors (no fallback)."""
import pytest
import torch

import uv_reference as U


def _fragments(p2f, bary):
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.renderer import Fragments
    return Fragments(p2f, torch.zeros(p2f.shape), bary, torch.zeros(p2f.shape))


def _triple(N=2, F=4, Vt=6, Hm=5, Wm=7, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(N, Hm, Wm, 3, generator=g), torch.randint(0, Vt, (N, F, 3), generator=g),
            torch.rand(N, Vt, 2, generator=g))


def test_construction_wrapper_to_clone_and_update_padded():
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.renderer import Textures, TexturesUV
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.structures import Meshes
    maps, fu, vu = _triple()
    a = TexturesUV(maps=maps, faces_uvs=fu, verts_uvs=vu)
    b = TexturesUV(maps=list(maps), faces_uvs=list(fu), verts_uvs=list(vu), padding_mode="zeros", align_corners=False)
    c = Textures(maps=maps, faces_uvs=fu, verts_uvs=vu)
    assert isinstance(c, TexturesUV)
    assert (a.padding_mode, a.align_corners) == ("border", True) == (c.padding_mode, c.align_corners)
    assert (b.padding_mode, b.align_corners) == ("zeros", False)
    for t in (a, b, c):
        assert torch.equal(t.maps_padded(), maps) and torch.equal(t.faces_uvs_padded(), fu)
        assert torch.equal(t.verts_uvs_padded(), vu)
        assert len(t.maps_list()) == len(t.faces_uvs_list()) == len(t.verts_uvs_list()) == 2
        assert torch.equal(t.maps_list()[1], maps[1]) and torch.equal(t.verts_uvs_list()[1], vu[1])
        assert torch.equal(t.faces_uvs_list()[0], fu[0])
    d = b.clone()
    assert isinstance(d, TexturesUV) and torch.equal(d.maps_padded(), maps)
    assert d.maps_padded().data_ptr() != maps.data_ptr() and (d.padding_mode, d.align_corners) == ("zeros", False)
    e = b.to("cpu")
    assert isinstance(e, TexturesUV) and e.device == torch.device("cpu") and e.padding_mode == "zeros"
    # faces_verts_uvs_packed is verts_uvs[faces_uvs] mesh after mesh, and carries the gradient to verts_uvs
    vg = vu.clone().requires_grad_(True)
    fv = TexturesUV(maps, fu, vg).faces_verts_uvs_packed()
    assert tuple(fv.shape) == (8, 3, 2) and torch.equal(fv[5], vu[1][fu[1, 1]])
    fv.sum().backward()
    assert float(vg.grad.sum()) == 2 * 4 * 3 * 2
    mesh = Meshes(verts=torch.rand(2, 6, 3), faces=fu, textures=a)
    assert mesh.update_padded(torch.rand(2, 6, 3)).textures is a
    assert isinstance(mesh.to("cpu").textures, TexturesUV)


def test_constructor_refusals():
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.renderer import TexturesUV
    maps, fu, vu = _triple()
    with pytest.raises(ValueError, match="3 channels"):
        TexturesUV(torch.rand(2, 5, 7, 4), fu, vu)
    bad = fu.clone()
    bad[1, 2, 0] = 6
    with pytest.raises(ValueError, match="out of range"):
        TexturesUV(maps, bad, vu)
    bad[1, 2, 0] = -1
    with pytest.raises(ValueError, match="out of range"):
        TexturesUV(maps, bad, vu)
    with pytest.raises(ValueError, match="equal size"):
        TexturesUV([maps[0], maps[1, :4]], fu, vu)
    with pytest.raises(ValueError, match="equal size"):
        TexturesUV(maps, [fu[0], fu[1, :3]], vu)
    with pytest.raises(ValueError, match="equal size"):
        TexturesUV(maps, fu, [vu[0], vu[1, :5]])
    with pytest.raises(ValueError, match="reflection"):
        TexturesUV(maps, fu, vu, padding_mode="reflection")
    with pytest.raises(ValueError, match="same, non-zero number of meshes"):
        TexturesUV(maps, fu[:1], vu)
    with pytest.raises(ValueError, match="align_corners"):
        TexturesUV(torch.rand(2, 1, 7, 3), fu, vu)
    with pytest.raises(ValueError, match="int64"):
        TexturesUV(maps, fu.int(), vu)


def _hand_fragments(N, H, W, K, F, seed):
    g = torch.Generator().manual_seed(seed)
    p2f = torch.randint(-1, F, (N, H, W, K), generator=g)
    p2f = torch.where(p2f >= 0, p2f + F * torch.arange(N).reshape(N, 1, 1, 1), p2f)
    bary = torch.rand(N, H, W, K, 3, generator=g)
    return p2f, bary / bary.sum(dim=-1, keepdim=True)


@pytest.mark.parametrize("padding_mode", ["border", "zeros"])
@pytest.mark.parametrize("align_corners", [True, False])
def test_host_sample_textures_equals_the_restatement(align_corners, padding_mode):
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.renderer import TexturesUV
    N, H, W, K, F, Vt, Hm, Wm = 2, 4, 5, 2, 4, 6, 5, 7
    maps, fu, _ = _triple(N, F, Vt, Hm, Wm, seed=3)
    vu = torch.rand(N, Vt, 2, generator=torch.Generator().manual_seed(4)) * 1.4 - 0.2   # some taps leave the map
    p2f, bary = _hand_fragments(N, H, W, K, F, 5)
    assert bool((p2f < 0).any()) and bool((p2f >= F).any())
    tex = TexturesUV(maps.double(), fu, vu.double(), padding_mode=padding_mode, align_corners=align_corners)
    got = tex.sample_textures(_fragments(p2f, bary.double()))
    fv = tex.faces_verts_uvs_packed()
    ref = U.restatement(p2f, bary.double(), fv, maps.double(), align_corners, padding_mode)
    assert tuple(got.shape) == (N, H, W, K, 3)
    assert float((got - ref).abs().max()) <= 1e-12
    assert float((U.composition(p2f, bary.double(), fv, maps.double(), align_corners, padding_mode) - ref).abs().max()) \
        <= 1e-12
    # the mesh is the pixel's: each half of the batch sees its own map only
    other = TexturesUV(torch.stack([maps[0], maps[1] + 1.0]).double(), fu, vu.double(), padding_mode=padding_mode,
                       align_corners=align_corners).sample_textures(_fragments(p2f, bary.double()))
    assert torch.equal(other[0], got[0]) and not torch.equal(other[1], got[1])


def test_empty_slots_hold_the_sample_at_uv_zero():
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.renderer import TexturesUV
    maps, fu, vu = _triple(seed=6)
    p2f = torch.full((2, 3, 3, 2), -1, dtype=torch.int64)
    bary = torch.full((2, 3, 3, 2, 3), -1.0)
    got = TexturesUV(maps, fu, vu).sample_textures(_fragments(p2f, bary))
    for n in range(2):
        assert torch.equal(got[n], maps[n, 4, 0].expand(3, 3, 2, 3))


@pytest.mark.parametrize("align_corners", [True, False])
def test_unit_quad_equals_grid_sample(align_corners):
    """One [0,1]^2 quad of two triangles whose UVs are its positions, sampled at a grid of points: sample_textures is
    grid_sample of the flipped map at 2 uv - 1."""
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.renderer import TexturesUV
    H, W, Hm, Wm = 6, 7, 5, 8
    maps = torch.rand(1, Hm, Wm, 3, generator=torch.Generator().manual_seed(7)).double()
    vu = torch.tensor([[[0., 0.], [1., 0.], [1., 1.], [0., 1.]]], dtype=torch.float64)
    fu = torch.tensor([[[0, 1, 2], [0, 2, 3]]])
    v, u = torch.meshgrid((torch.arange(H, dtype=torch.float64) + 0.5) / H,
                          (torch.arange(W, dtype=torch.float64) + 0.25) / W, indexing="ij")
    lower = u >= v
    bary = torch.where(lower[..., None], torch.stack([1 - u, u - v, v], -1), torch.stack([1 - v, u, v - u], -1))
    p2f = torch.where(lower, 0, 1)[None, ..., None]
    got = TexturesUV(maps, fu, vu, align_corners=align_corners).sample_textures(_fragments(p2f, bary[None, :, :, None]))
    grid = torch.stack([2 * u - 1, 2 * v - 1], -1)[None]
    ref = torch.nn.functional.grid_sample(torch.flip(maps, [1]).permute(0, 3, 1, 2), grid, mode="bilinear",
                                          padding_mode="border", align_corners=align_corners)
    assert float((got[0, :, :, 0] - ref[0].permute(1, 2, 0)).abs().max()) <= 1e-12


def test_uv_texels_checks_shapes_then_refuses_host_tensors():
    from acfm_video_3d_reconstruction_amd import ops
    p2f = torch.zeros(2, 4, 4, 2, dtype=torch.int64)
    bary, fv, maps = torch.zeros(2, 4, 4, 2, 3), torch.zeros(8, 3, 2), torch.zeros(2, 5, 7, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.uv_texels(p2f, bary, fv, maps)
    for args, kw, what in (
            ((torch.zeros(2, 4, 4, 5, dtype=torch.int64), torch.zeros(2, 4, 4, 5, 3), fv, maps), {}, "faces_per_pixel"),
            ((p2f, torch.zeros(2, 4, 4, 2, 2), fv, maps), {}, "bary_coords"),
            ((p2f, bary, torch.zeros(8, 3, 3), maps), {}, "faces_verts_uvs"),
            ((p2f, bary, fv, torch.zeros(3, 5, 7, 3)), {}, "maps"),
            ((p2f, bary, fv, torch.zeros(2, 5, 7, 4)), {}, "maps"),
            ((p2f, bary, fv, torch.zeros(2, 1, 7, 3)), {}, "align_corners"),
            ((p2f, bary, fv, maps), {"padding_mode": "reflection"}, "reflection"),
            ((p2f, bary, fv, maps.half()), {}, "float32"),
            ((p2f, bary.double(), fv, maps), {}, "float32")):
        with pytest.raises(ValueError, match=what):
            ops.uv_texels(*args, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.uv_texels(p2f, bary, fv, torch.zeros(2, 1, 7, 3), align_corners=False)
