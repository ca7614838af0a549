"""pytorch3d.renderer.mesh.shading (0.3.0): phong_shading, gouraud_shading and flat_shading.

On GPU float32 tensors, with lights, materials and camera that need no gradient, the three run on the lit kernels
(ops.phong_shade, ops.light_points): position and normal are interpolated inside the shader kernel, nothing of size
[N,H,W,K,3] exists besides the texels and the colours.  Every other case -- host tensors, a light, material or camera
tensor that requires a gradient, a K outside ops.FRAGMENT_K -- runs the composition of torch operators around
interpolate_face_attributes, which is also the statement of the definition: `with fused(False):` forces it."""
import torch

from .... import ops as _ops
from ..lighting import DirectionalLights, PointLights
from .textures import interpolate_face_attributes as _interpolate

_FUSED = [True]   # (a one-element list: mutated in place, never rebound)


class fused:
    """with fused(False): ...  -- the shading functions called inside the block run the composition of torch
    operators even where the fused kernels apply (the comparison of the tests and of tools/phong_bench.py);
    fused(True) restores the default inside such a block."""

    def __init__(self, on=True):
        self.on = bool(on)

    def __enter__(self):
        self.prev, _FUSED[0] = _FUSED[0], self.on
        return self

    def __exit__(self, *exc):
        _FUSED[0] = self.prev


def _apply_lighting(points, normals, lights, cameras, materials, **kwargs):
    light_diffuse = lights.diffuse(normals=normals, points=points)
    light_specular = lights.specular(normals=normals, points=points,
                                     camera_position=cameras.get_camera_center(**kwargs),
                                     shininess=materials.shininess)
    n = normals.dim()
    per_mesh = lambda t: t.reshape((t.shape[0],) + (1,) * (n - 2) + (3,))
    ambient_color = per_mesh(materials.ambient_color * lights.ambient_color)
    diffuse_color = per_mesh(materials.diffuse_color) * light_diffuse
    specular_color = per_mesh(materials.specular_color) * light_specular
    return ambient_color, diffuse_color, specular_color


def _camera_centre(cameras, kwargs):
    """cameras.get_camera_center, C R + T = 0, with the 3 x 3 inverse in closed form (rows of R crossed, over the
    determinant): no LAPACK call and no host read, so the fused path stays capturable into a hipGraph."""
    w2v = cameras.get_world_to_view_transform(**kwargs)
    R, T = w2v.R, w2v.T
    r0, r1, r2 = R[:, 0], R[:, 1], R[:, 2]
    cof = torch.stack([torch.cross(r1, r2, dim=-1), torch.cross(r2, r0, dim=-1), torch.cross(r0, r1, dim=-1)], 1)
    det = (r0 * cof[:, 0]).sum(-1, keepdim=True)
    return -(cof * T[:, None, :]).sum(-1) / det


def _light_constants(meshes, fragments, lights, cameras, materials, tensors, kwargs):
    """ops.LightConstants of the fused path, or None where the composition has to run: fused(False), host or
    non-float32 tensors, a K outside FRAGMENT_K, other images than meshes, a light class other than the two of
    lighting.py, or a light, material or camera tensor that requires a gradient."""
    if not _FUSED[0]:
        return None
    p2f = fragments.pix_to_face
    N = len(meshes)
    if p2f.dim() != 4 or p2f.shape[0] != N or p2f.numel() == 0 or int(p2f.shape[-1]) not in _ops.FRAGMENT_K:
        return None
    if isinstance(lights, PointLights):
        vector, point = lights.location, True
    elif isinstance(lights, DirectionalLights):
        vector, point = lights.direction, False
    else:
        return None
    for t in tensors + (fragments.bary_coords,):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32):
            return None
    if not hasattr(cameras, "get_world_to_view_transform"):
        return None
    centre = _camera_centre(cameras, kwargs)
    parts = (materials.ambient_color * lights.ambient_color, materials.diffuse_color * lights.diffuse_color,
             materials.specular_color * lights.specular_color, vector, centre)
    shininess = materials.shininess
    if any(t.requires_grad or not t.is_cuda or t.numel() not in (3, 3 * N) for t in parts):
        return None
    if torch.is_tensor(shininess) and (shininess.requires_grad or shininess.numel() not in (1, N)):
        return None
    return _ops.light_constants(*parts, shininess, N, point)


def phong_shading_composition(meshes, fragments, lights, cameras, materials, texels, **kwargs):
    """phong_shading as PyTorch3D 0.3.0 composes it: two interpolate_face_attributes and the lighting terms in torch."""
    verts = meshes.verts_packed()
    faces = meshes.faces_packed()
    vertex_normals = meshes.verts_normals_packed()
    pixel_coords = _interpolate(fragments.pix_to_face, fragments.bary_coords, verts[faces])
    pixel_normals = _interpolate(fragments.pix_to_face, fragments.bary_coords, vertex_normals[faces])
    ambient, diffuse, specular = _apply_lighting(pixel_coords, pixel_normals, lights, cameras, materials, **kwargs)
    return (ambient + diffuse) * texels + specular


def phong_shading(meshes, fragments, lights, cameras, materials, texels, **kwargs):
    """-> colors [N,H,W,K,3] = (ambient + diffuse) * texels + specular, at the interpolated pixel positions and
    vertex normals.  kwargs (R= / T=) reach cameras.get_camera_center."""
    if torch.is_tensor(texels) and texels.shape[-1] == 3:
        verts = meshes.verts_packed()
        lc = _light_constants(meshes, fragments, lights, cameras, materials, (verts, texels), kwargs)
        if lc is not None:
            return _ops.phong_shade(fragments, verts, meshes.faces_packed(), meshes.verts_normals_packed(), texels, lc,
                                    meshes.incidence_table_packed(), mode="phong")
    return phong_shading_composition(meshes, fragments, lights, cameras, materials, texels, **kwargs)


def gouraud_shading(meshes, fragments, lights, cameras, materials, **kwargs):
    """-> colors [N,H,W,K,3]: the vertex colours (meshes.textures.verts_features_packed()) lit AT THE VERTICES with the
    vertex normals, colour * (ambient + diffuse) + specular, then interpolated over the faces."""
    if not hasattr(meshes.textures, "verts_features_packed"):
        raise ValueError("gouraud_shading: meshes must have a TexturesVertex")
    faces = meshes.faces_packed()
    verts = meshes.verts_packed()
    colours = meshes.textures.verts_features_packed()
    lc = None
    if colours.shape[-1] == 3:
        lc = _light_constants(meshes, fragments, lights, cameras, materials, (verts, colours), kwargs)
    if lc is not None:
        lit = _ops.light_points(verts, meshes.verts_normals_packed(), colours, lc, meshes.verts_packed_to_mesh_idx())
    else:
        N = len(meshes)      # per mesh, so that the [N,3] light terms broadcast: [N,V,3]
        ambient, diffuse, specular = _apply_lighting(meshes.verts_padded(), meshes.verts_normals_padded(), lights,
                                                     cameras, materials, **kwargs)
        lit = (colours.reshape(N, -1, colours.shape[-1]) * (ambient + diffuse) + specular).reshape(-1, 3)
    return _interpolate(fragments.pix_to_face, fragments.bary_coords, lit[faces])


def flat_shading(meshes, fragments, lights, cameras, materials, texels, **kwargs):
    """-> colors [N,H,W,K,3] = (ambient + diffuse) * texels + specular at each face's centre and face normal (0 and 0
    in empty slots)."""
    verts = meshes.verts_packed()
    faces = meshes.faces_packed()
    face_normals = meshes.faces_normals_packed()
    if torch.is_tensor(texels) and texels.shape[-1] == 3:
        lc = _light_constants(meshes, fragments, lights, cameras, materials, (verts, texels), kwargs)
        if lc is not None:
            return _ops.phong_shade(fragments, verts, faces, face_normals, texels, lc, meshes.incidence_table_packed(),
                                    mode="flat")
    face_coords = verts[faces].mean(dim=-2)
    p2f = fragments.pix_to_face
    empty = (p2f < 0)[..., None]
    idx = p2f.clamp(min=0)
    pixel_coords = torch.where(empty, torch.zeros_like(face_coords[idx]), face_coords[idx])
    pixel_normals = torch.where(empty, torch.zeros_like(face_normals[idx]), face_normals[idx])
    ambient, diffuse, specular = _apply_lighting(pixel_coords, pixel_normals, lights, cameras, materials, **kwargs)
    return (ambient + diffuse) * texels + specular
