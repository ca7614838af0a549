"""pytorch3d.renderer.mesh.shading (0.3.0): phong_shading.  Pixel positions and normals come from the HIP
interpolate_face_attributes; the lighting terms are torch."""
from .... import ops as _ops


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


def phong_shading(meshes, fragments, lights, cameras, materials, texels, **kwargs):
    """-> colors [N,H,W,K,3] = (ambient + diffuse) * texels + specular, at the interpolated pixel positions and
    vertex normals.  kwargs (R= / T=) reach cameras.get_camera_center."""
    verts = meshes.verts_packed()
    faces = meshes.faces_packed()
    vertex_normals = meshes.verts_normals_packed()
    pixel_coords = _ops.interpolate_face_attributes(fragments.pix_to_face, fragments.bary_coords, verts[faces])
    pixel_normals = _ops.interpolate_face_attributes(fragments.pix_to_face, fragments.bary_coords,
                                                     vertex_normals[faces])
    ambient, diffuse, specular = _apply_lighting(pixel_coords, pixel_normals, lights, cameras, materials, **kwargs)
    return (ambient + diffuse) * texels + specular
