"""pytorch3d.renderer.mesh (0.3.0): the rasterizer."""
from . import rasterize_meshes as _rasterize_meshes_module  # noqa: F401
from . import rasterizer  # noqa: F401
from .rasterize_meshes import rasterize_meshes  # noqa: F401
from .rasterizer import Fragments, MeshRasterizer, RasterizationSettings  # noqa: F401
