"""pytorch3d.renderer.mesh (0.3.0): the rasterizer, textures, shading, shaders and MeshRenderer."""
from . import rasterize_meshes as _rasterize_meshes_module  # noqa: F401
from . import rasterizer, renderer, shader, shading, textures  # noqa: F401
from .rasterize_meshes import rasterize_meshes  # noqa: F401
from .rasterizer import Fragments, MeshRasterizer, RasterizationSettings  # noqa: F401
from .renderer import MeshRenderer  # noqa: F401
from .shader import (HardFlatShader, HardGouraudShader, HardPhongShader, SoftGouraudShader,  # noqa: F401
                     SoftPhongShader, SoftSilhouetteShader, TexturedSoftPhongShader)
from .shading import flat_shading, gouraud_shading, phong_shading  # noqa: F401
from .textures import Textures, TexturesAtlas, TexturesUV, TexturesVertex  # noqa: F401
