"""The slice of the PyTorch3D 0.3.0 API that the reference's callers import
(multiframe/main.py:29-38, nnutils/predictor.py:9,21,64, nnutils/mesh_net.py:16):
`structures.Meshes`, `loss.mesh_laplacian_smoothing`, `ops.SubdivideMeshes`, `io.load_obj`, and what
utils/geometry.py:63-72 imports for the template fit (`io.save_obj`, `utils.ico_sphere`,
`ops.sample_points_from_meshes`, `loss.{chamfer_distance, mesh_edge_loss, mesh_normal_consistency}`),
PyTorch3D 0.3.0's point-set pair `ops.{knn_points, knn_gather}`,
`transforms.{standardize_quaternion, quaternion_multiply, matrix_to_quaternion, ...}`.

It is a shape-compatible shim (same names, arguments, return types), not PyTorch3D.  Of the
renderer, `renderer` holds the rasterizer (`rasterize_meshes`, `MeshRasterizer`, `Fragments`,
`RasterizationSettings`, `SfMOrthographicCameras`, `look_at_view_transform`) on the HIP kernels;
and the shading half over its Fragments (`BlendParams`, the blends, lights, materials, `TexturesAtlas` /
`TexturesVertex` / `Textures`, the shaders and `MeshRenderer`), so the reference's `MeshRenderer(MeshRasterizer,
shader)` compositions run as written; nnutils.nmr keeps the hand-fused renders of its two fixed settings.
`install()` registers the shim as the `pytorch3d` package so `from pytorch3d.structures import
Meshes` in unmodified caller code resolves to it when the real package is absent."""
import sys

from . import io, loss, ops, renderer, structures, transforms, utils  # noqa: F401

_RENDERER_MODULES = ("renderer", "renderer.blending", "renderer.cameras", "renderer.lighting", "renderer.materials",
                     "renderer.mesh", "renderer.mesh.rasterizer", "renderer.mesh.rasterize_meshes",
                     "renderer.mesh.renderer", "renderer.mesh.shader", "renderer.mesh.shading",
                     "renderer.mesh.textures")


def install(force=False):
    if "pytorch3d" in sys.modules and not force:
        return sys.modules["pytorch3d"]
    me = sys.modules[__name__]
    sys.modules["pytorch3d"] = me
    for name in ("io", "loss", "ops", "structures", "transforms", "utils"):
        sys.modules["pytorch3d." + name] = getattr(me, name)
    for name in _RENDERER_MODULES:
        sys.modules["pytorch3d." + name] = sys.modules[__name__ + "." + name]
    return me
