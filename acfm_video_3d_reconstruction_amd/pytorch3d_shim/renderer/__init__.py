"""pytorch3d.renderer of PyTorch3D 0.3.0, the rasterizer slice: `rasterize_meshes`, `Fragments`,
`RasterizationSettings`, `MeshRasterizer`, `SfMOrthographicCameras`, `look_at_view_transform`.
The camera maths is torch (differentiable through autograd); the raster is ops.rasterize_fragments on
the HIP kernels.  No shaders here."""
from . import cameras, mesh  # noqa: F401
from .cameras import SfMOrthographicCameras, look_at_rotation, look_at_view_transform  # noqa: F401
from .mesh import Fragments, MeshRasterizer, RasterizationSettings, rasterize_meshes  # noqa: F401
