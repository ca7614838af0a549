"""Host only: the lit shading of the shim on host tensors (gouraud_shading, flat_shading and the Gouraud / flat
shaders, which run the composition of torch operators there) against the float64 restatements of lit_reference.py;
install(); the vertex-to-corner incidence table."""
import numpy as np
import pytest
import torch

import lit_reference as R

N, H, K = 2, 16, 2
AMB, DIF, SPEC = (0.3, 0.25, 0.2), (0.6, 0.5, 0.4), (0.2, 0.3, 0.25)
VEC = {False: (0.3, 1.0, -1.0), True: (0.5, 1.0, -2.0)}
T = (0.0, 0.0, 2.732)
SHININESS = 10
BG = (0.2, 0.5, 0.9)
GAMMA = 1.0


def _scene(seed):
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.utils import ico_sphere
    s = ico_sphere(1)
    v0, f = s.verts_packed(), s.faces_packed()
    g = torch.Generator().manual_seed(seed)
    verts = (v0[None] + 0.05 * torch.randn(N, v0.shape[0], 3, generator=g)).float()
    colours = torch.rand(N, v0.shape[0], 3, generator=g)
    p2f, zbuf, bary, dists, g = R.fragments(N, H, H, K, f.shape[0], seed + 1)
    texels = torch.rand(N, H, H, K, 3, generator=g)
    return verts, f, colours, (p2f, zbuf, bary, dists), texels, g


def _parts(point):
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.renderer import (DirectionalLights, Materials, PointLights,
                                                                          SfMOrthographicCameras)
    kw = dict(ambient_color=(AMB,), diffuse_color=(DIF,), specular_color=(SPEC,))
    lights = PointLights(location=(VEC[True],), **kw) if point else DirectionalLights(direction=(VEC[False],), **kw)
    cam = SfMOrthographicCameras(T=torch.tensor([T]))
    # the camera's view is X R + T with R = 1: its centre is -T
    ref = R.Light(N, AMB, DIF, SPEC, VEC[point], point, tuple(-t for t in T), SHININESS)
    return lights, cam, Materials(shininess=SHININESS), ref


def _meshes(verts, faces, colours):
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.renderer import TexturesVertex
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.structures import Meshes
    v, c = verts.clone().requires_grad_(True), colours.clone().requires_grad_(True)
    return Meshes(verts=v, faces=faces[None].expand(N, -1, -1), textures=TexturesVertex(c)), v, c


def _packed_faces(faces, V):
    return torch.cat([faces + n * V for n in range(N)], 0)


def _check(got, ref, G, leaves, ref_leaves, what):
    R.close(got, ref, floor=0.0, what=what + " colours", scale_bar=1e-6, rel_l2=1e-6)
    grads = torch.autograd.grad((got * G).sum(), leaves)
    refs = torch.autograd.grad((ref * G.double()).sum(), ref_leaves)
    for g, r, name in zip(grads, refs, ("verts", "colours")):
        R.close(g, r, floor=1e-9, what="%s grad %s" % (what, name))


@pytest.mark.parametrize("point", [False, True], ids=["directional", "point"])
def test_host_shading_vs_float64(point):
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.renderer import Fragments
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.renderer.mesh.shading import flat_shading, gouraud_shading
    verts, faces, colours, planes, texels, g = _scene(10 + point)
    lights, cam, mat, ref_light = _parts(point)
    fr = Fragments(*planes)
    p2f, bary = planes[0], planes[2].double()
    pf = _packed_faces(faces, verts.shape[1])
    G = torch.randn(N, H, H, K, 3, generator=g)

    mesh, v, c = _meshes(verts, faces, colours)
    rv, rc = verts.double().requires_grad_(True), colours.double().requires_grad_(True)
    _check(gouraud_shading(mesh, fr, lights, cam, mat), R.gouraud(rv, pf, rc, p2f, bary, ref_light), G, (v, c), (rv, rc),
           "gouraud")

    # flat: the texels are the interpolated vertex colours, so both leaves receive a gradient
    mesh, v, c = _meshes(verts, faces, colours)
    rv, rc = verts.double().requires_grad_(True), colours.double().requires_grad_(True)
    got = flat_shading(mesh, fr, lights, cam, mat, mesh.sample_textures(fr))
    ref = R.shade("flat", rv.reshape(-1, 3), pf, p2f, bary, R.interpolate(p2f, bary, rc.reshape(-1, 3)[pf]), ref_light)
    _check(got, ref, G, (v, c), (rv, rc), "flat")


@pytest.mark.parametrize("point", [False, True], ids=["directional", "point"])
def test_host_shaders_vs_float64(point):
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.renderer import (BlendParams, Fragments, HardFlatShader,
                                                                          HardGouraudShader, SoftGouraudShader)
    verts, faces, colours, planes, texels, g = _scene(20 + point)
    lights, cam, mat, ref_light = _parts(point)
    fr = Fragments(*planes)
    p2f, zbuf, bary, dists = (t.double() if t.is_floating_point() else t for t in planes)
    pf = _packed_faces(faces, verts.shape[1])
    # gamma = 1: the soft blend's weights are exp((z - z_max) / gamma), whose float32 rounding is eps / gamma relative
    # (6e-6 at gamma = 1e-2, above the 1e-6 colour bar whatever the shading does); the blend itself is not under test
    bp = BlendParams(1e-4, GAMMA, BG)
    G = torch.randn(N, H, H, 4, generator=g)
    kw = dict(cameras=cam, lights=lights, materials=mat, blend_params=bp)
    for cls in (SoftGouraudShader, HardGouraudShader, HardFlatShader):
        mesh, v, c = _meshes(verts, faces, colours)
        rv, rc = verts.double().requires_grad_(True), colours.double().requires_grad_(True)
        got = cls(**kw)(fr, mesh)
        if cls is HardFlatShader:
            cols = R.shade("flat", rv.reshape(-1, 3), pf, p2f, bary, R.interpolate(p2f, bary, rc.reshape(-1, 3)[pf]),
                           ref_light)
        else:
            cols = R.gouraud(rv, pf, rc, p2f, bary, ref_light)
        ref = R.softmax_blend(p2f, dists, zbuf, cols, 1e-4, GAMMA, BG) if cls is SoftGouraudShader else \
            R.hard_blend(p2f, cols, BG)
        assert tuple(got.shape) == (N, H, H, 4)
        _check(got, ref, G, (v, c), (rv, rc), cls.__name__)


def test_install_exports_the_new_shaders():
    import sys
    from acfm_video_3d_reconstruction_amd import pytorch3d_shim
    saved = {k: m for k, m in sys.modules.items() if k == "pytorch3d" or k.startswith("pytorch3d.")}
    try:
        pytorch3d_shim.install(force=True)
        from pytorch3d.renderer import HardFlatShader, HardGouraudShader, SoftGouraudShader
        from pytorch3d.renderer.mesh.shader import HardFlatShader as H2
        from pytorch3d.renderer.mesh.shading import flat_shading, gouraud_shading, phong_shading  # noqa: F401
        assert H2 is HardFlatShader and SoftGouraudShader is not HardGouraudShader
    finally:
        for k in [k for k in sys.modules if k == "pytorch3d" or k.startswith("pytorch3d.")]:
            del sys.modules[k]
        sys.modules.update(saved)


def test_incidence_table():
    """Ascending by face, every corner exactly once, right on a mesh with an unreferenced vertex and a hub."""
    from acfm_video_3d_reconstruction_amd import ops
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.structures import Meshes
    faces = torch.tensor([[0, 1, 2], [0, 2, 3], [5, 0, 3], [2, 1, 5]])      # vertex 4 is in no face
    t = ops.incidence_table(faces, 7)                                       # ... nor is vertex 6, the last one
    off, cor = t.offsets.numpy(), t.corners.numpy()
    assert off.dtype == np.int32 and cor.dtype == np.int32 and off.shape == (8,) and cor.shape == (12,)
    assert off[0] == 0 and off[-1] == 12 and (np.diff(off) >= 0).all()
    assert sorted(cor.tolist()) == list(range(12))
    flat = faces.reshape(-1).numpy()
    for v in range(7):
        row = cor[off[v]:off[v + 1]]
        assert (flat[row] == v).all() and (np.diff(row) > 0).all() and len(row) == int((flat == v).sum())
    assert off[5] == off[4] and off[7] == off[6]
    vf, ff = R.fan(64)
    t = ops.incidence_table(ff, vf.shape[0])
    assert int(t.offsets[1]) - int(t.offsets[0]) == 64
    assert t.corners[:64].tolist() == [3 * f for f in range(64)]
    # Meshes memoises it on the faces tensor: a second Meshes around the same faces gets the same tensors
    m1 = Meshes(verts=vf[None], faces=ff[None])
    m2 = Meshes(verts=vf[None] * 2, faces=m1.faces_padded())
    assert m1.incidence_table_packed().corners is m2.incidence_table_packed().corners
    assert torch.equal(m1.incidence_table_packed().offsets, t.offsets)


# ------------------------------------------------------------------------------------------------ vis.py host math
def test_rodrigues_closed_forms():
    from acfm_video_3d_reconstruction_amd import vis
    forms = {0: lambda c, s: [[1, 0, 0], [0, c, -s], [0, s, c]],
             1: lambda c, s: [[c, 0, s], [0, 1, 0], [-s, 0, c]],
             2: lambda c, s: [[c, -s, 0], [s, c, 0], [0, 0, 1]]}
    for axis in range(3):
        for deg, (c, s) in ((0, (1.0, 0.0)), (90, (0.0, 1.0)), (180, (-1.0, 0.0))):
            r = np.zeros(3)
            r[axis] = np.deg2rad(deg)
            assert np.allclose(vis.rodrigues(r), np.array(forms[axis](c, s), dtype=np.float64), atol=1e-12), (axis, deg)
    R = vis.rodrigues([0.3, -0.2, 0.9])
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-12) and abs(np.linalg.det(R) - 1.0) < 1e-12


def test_matrix_quaternion_round_trip():
    from acfm_video_3d_reconstruction_amd import vis
    rng = np.random.default_rng(0)
    vecs = [rng.normal(size=3) for _ in range(20)]
    vecs += [np.pi * np.eye(3)[i] for i in range(3)]                 # half turns: the trace is -1, w = 0
    vecs += [np.zeros(3), [np.pi / 3, 0, 0], [0, np.pi / 2, 0]]
    for r in vecs:
        R = vis.rodrigues(r)
        q = vis.quaternion_from_matrix(R)
        assert abs(np.linalg.norm(q) - 1.0) < 1e-12 and q[0] >= 0.0
        assert np.allclose(vis.quaternion_matrix(q), R, atol=1e-12)
        R4 = np.eye(4)
        R4[:3, :3] = R
        assert np.allclose(vis.quaternion_from_matrix(R4), q, atol=1e-15)
    assert np.allclose(vis.quaternion_from_matrix(np.eye(3)), [1, 0, 0, 0])
    cam = vis.default_camera()
    assert cam.dtype == np.float32 and np.allclose(cam[:3], [0.75, 0, 0])
    side = vis.rodrigues([0, np.pi / 2, 0]) @ vis.rodrigues([np.pi / 3, 0, 0])
    assert np.allclose(vis.quaternion_matrix(cam[3:]), side, atol=1e-6)
    assert np.allclose(vis.DEFAULT_COLOUR, np.array([156, 199, 234]) / 255.0)


def test_diff_vp_camera_is_rotate_by_times_r():
    from acfm_video_3d_reconstruction_amd import vis
    cam = np.concatenate([[0.9, 0.1, -0.2], vis.quaternion_from_matrix(vis.rodrigues([0.4, -0.7, 0.2]))])
    R = vis.quaternion_matrix(cam[3:])
    for angle, axis, elev in ((90, (1, 0, 0), False), (-30, (0, 1, 0), False), (45, (0, 0, 1), True)):
        new = vis.viewpoint_camera(cam, angle, axis, None, elev)
        want = vis.rodrigues(np.deg2rad(angle) * np.array(axis, dtype=np.float64)) @ R
        if elev:
            want = vis.rodrigues([np.pi / 9, 0, 0]) @ want
        assert np.allclose(new[:3], [0.6, 0, 0]) and new.dtype == np.float32
        assert np.allclose(vis.quaternion_matrix(new[3:]), want, atol=1e-6)
    assert np.allclose(vis.viewpoint_camera(cam, 10, (1, 0, 0), [0.5, 0.1, 0.2])[:3], [0.5, 0.1, 0.2])
