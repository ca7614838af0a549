"""pytorch3d.renderer of PyTorch3D 0.3.0: the rasterizer (`rasterize_meshes`, `Fragments`, `RasterizationSettings`,
`MeshRasterizer`, `SfMOrthographicCameras`, `look_at_view_transform`) and the shading half (`BlendParams` and the
blends, `DirectionalLights` / `PointLights`, `Materials`, `TexturesAtlas` / `TexturesVertex` / `Textures`, the
shaders and `MeshRenderer`).  Camera and lighting maths is torch (differentiable through autograd); the raster, the
blends, the attribute interpolation and the lit shading (Phong, Gouraud, flat) are HIP kernels
(ops.rasterize_fragments and the shader ops)."""
from . import blending, cameras, lighting, materials, mesh  # noqa: F401
from .blending import BlendParams, hard_rgb_blend, sigmoid_alpha_blend, softmax_rgb_blend  # noqa: F401
from .cameras import SfMOrthographicCameras, look_at_rotation, look_at_view_transform  # noqa: F401
from .lighting import DirectionalLights, PointLights  # noqa: F401
from .materials import Materials  # noqa: F401
from .mesh import (Fragments, HardFlatShader, HardGouraudShader, HardPhongShader, MeshRasterizer,  # noqa: F401
                   MeshRenderer, RasterizationSettings, SoftGouraudShader, SoftPhongShader, SoftSilhouetteShader, Textures, TexturedSoftPhongShader, TexturesAtlas,
                   TexturesUV, TexturesVertex, rasterize_meshes)
