"""pytorch3d.renderer.mesh.rasterize_meshes (0.3.0) on ops.rasterize_fragments."""
from .... import ops as _ops


def _square_size(image_size):
    if isinstance(image_size, (tuple, list)):
        if len(image_size) != 2 or int(image_size[0]) != int(image_size[1]):
            raise ValueError("image_size: only square images are supported, got %r" % (tuple(image_size),))
        return int(image_size[0])
    return int(image_size)


def check_raster_options(image_size=256, faces_per_pixel=8, perspective_correct=False, cull_backfaces=False):
    """The options the HIP rasterizer does not implement raise here, by name."""
    if perspective_correct:
        raise ValueError("perspective_correct=True is not supported (orthographic cameras only)")
    if cull_backfaces:
        raise ValueError("cull_backfaces=True is not supported")
    if int(faces_per_pixel) not in _ops.FRAGMENT_K:
        raise ValueError("faces_per_pixel=%r is not supported (one of %s)" % (faces_per_pixel, _ops.FRAGMENT_K))
    return _square_size(image_size)


def rasterize_meshes(meshes, image_size=256, blur_radius=0.0, faces_per_pixel=8, bin_size=None,
                     max_faces_per_bin=None, perspective_correct=False, clip_barycentric_coords=False,
                     cull_backfaces=False):
    """Rasterize a batch of meshes whose vertices are already in NDC / view space (x, y in NDC, z the view depth).

    -> (pix_to_face [N,H,H,K] int64, zbuf [N,H,H,K], bary_coords [N,H,H,K,3], dists [N,H,H,K]), -1 in empty slots,
    with PyTorch3D's semantics: pix_to_face indexes the packed faces, zbuf is the interpolated view z, dists the
    squared distance to the nearest edge (negative inside), bary_coords clamped to [0, 1] and renormalised when
    clip_barycentric_coords is set.  zbuf, bary_coords and dists carry gradients to the vertices.

    bin_size and max_faces_per_bin are accepted and ignored: the outputs are those of the naive path (what the
    coarse-to-fine path of PyTorch3D computes too, short of bin overflow), which is what the project's oracle
    restates.  Not supported (ValueError naming the argument): perspective_correct=True, cull_backfaces=True, a
    non-square image_size, meshes of different vertex or face counts in one batch, faces_per_pixel outside
    ops.FRAGMENT_K."""
    del bin_size, max_faces_per_bin
    H = check_raster_options(image_size, faces_per_pixel, perspective_correct, cull_backfaces)
    if not meshes._equal_sized():
        raise ValueError("meshes: every mesh of the batch must have the same number of vertices and of faces")
    return _ops.rasterize_fragments(meshes.verts_padded(), meshes.faces_padded(), H, int(faces_per_pixel),
                                    blur_radius=float(blur_radius), clip_barycentric_coords=bool(clip_barycentric_coords))
