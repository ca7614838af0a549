"""pytorch3d.renderer.mesh.shader (0.3.0): SoftSilhouetteShader, SoftPhongShader (TexturedSoftPhongShader is its 0.3.0
alias), HardPhongShader, SoftGouraudShader, HardGouraudShader and HardFlatShader.  forward(fragments, meshes, **kwargs) accepts cameras= / lights= / materials= /
blend_params= overrides.  SoftPhongShader with ambient-only lights and a TexturesAtlas -- the reference's texture
configuration -- takes ops.atlas_softmax_blend (texels sampled inside the blend kernel); every other combination
goes through phong_shading and the dense softmax kernel.  The Gouraud and flat shaders are restated from memory of
0.3.0's shader.py (the package is not at hand): Gouraud lights the TexturesVertex colours at the vertices, flat shades
each fragment at its face's centre and face normal."""
from torch import nn

from .... import ops as _ops
from ..blending import BlendParams, hard_rgb_blend, sigmoid_alpha_blend, softmax_rgb_blend
from ..lighting import PointLights
from ..materials import Materials
from .shading import flat_shading, gouraud_shading, phong_shading
from .textures import TexturesAtlas


class _Shader(nn.Module):
    def __init__(self, device="cpu", cameras=None, lights=None, materials=None, blend_params=None):
        super().__init__()
        self.lights = lights if lights is not None else PointLights(device=device)
        self.materials = materials if materials is not None else Materials(device=device)
        self.cameras = cameras
        self.blend_params = blend_params if blend_params is not None else BlendParams()

    def to(self, device):
        if self.cameras is not None:
            self.cameras = self.cameras.to(device)
        self.lights = self.lights.to(device)
        self.materials = self.materials.to(device)
        return self

    def _parts(self, kwargs):
        cameras = kwargs.get("cameras", self.cameras)
        if cameras is None:
            raise ValueError("Cameras must be specified either at initialization or in the forward pass of %s"
                             % type(self).__name__)
        return (cameras, kwargs.get("lights", self.lights), kwargs.get("materials", self.materials),
                kwargs.get("blend_params", self.blend_params))

    @staticmethod
    def _view(kwargs):
        return {k: kwargs[k] for k in ("R", "T") if k in kwargs}


class SoftSilhouetteShader(nn.Module):
    def __init__(self, blend_params=None):
        super().__init__()
        self.blend_params = blend_params if blend_params is not None else BlendParams()

    def forward(self, fragments, meshes, **kwargs):
        """-> [N,H,W,4]: RGB 1, alpha the soft silhouette (the sigmoid kernel without a colour tensor)."""
        return sigmoid_alpha_blend(None, fragments, kwargs.get("blend_params", self.blend_params))


class SoftPhongShader(_Shader):
    def forward(self, fragments, meshes, **kwargs):
        cameras, lights, materials, blend_params = self._parts(kwargs)
        znear = kwargs.get("znear", getattr(cameras, "znear", 1.0))
        zfar = kwargs.get("zfar", getattr(cameras, "zfar", 100.0))
        tex = meshes.textures
        ambient = materials.ambient_color * lights.ambient_color
        if isinstance(tex, TexturesAtlas) and not ambient.requires_grad and lights.no_diffuse_or_specular():
            return _ops.atlas_softmax_blend(tex.atlas_padded(), fragments, blend_params, ambient=ambient, znear=znear,
                                            zfar=zfar)
        texels = meshes.sample_textures(fragments)
        colors = phong_shading(meshes=meshes, fragments=fragments, texels=texels, lights=lights, cameras=cameras,
                               materials=materials, **self._view(kwargs))
        return softmax_rgb_blend(colors, fragments, blend_params, znear=znear, zfar=zfar)


TexturedSoftPhongShader = SoftPhongShader


class HardPhongShader(_Shader):
    def forward(self, fragments, meshes, **kwargs):
        cameras, lights, materials, blend_params = self._parts(kwargs)
        texels = meshes.sample_textures(fragments)
        colors = phong_shading(meshes=meshes, fragments=fragments, texels=texels, lights=lights, cameras=cameras,
                               materials=materials, **self._view(kwargs))
        return hard_rgb_blend(colors, fragments, blend_params)


class SoftGouraudShader(_Shader):
    def forward(self, fragments, meshes, **kwargs):
        cameras, lights, materials, blend_params = self._parts(kwargs)
        znear = kwargs.get("znear", getattr(cameras, "znear", 1.0))
        zfar = kwargs.get("zfar", getattr(cameras, "zfar", 100.0))
        colors = gouraud_shading(meshes=meshes, fragments=fragments, lights=lights, cameras=cameras,
                                 materials=materials, **self._view(kwargs))
        return softmax_rgb_blend(colors, fragments, blend_params, znear=znear, zfar=zfar)


class HardGouraudShader(_Shader):
    def forward(self, fragments, meshes, **kwargs):
        cameras, lights, materials, blend_params = self._parts(kwargs)
        colors = gouraud_shading(meshes=meshes, fragments=fragments, lights=lights, cameras=cameras,
                                 materials=materials, **self._view(kwargs))
        return hard_rgb_blend(colors, fragments, blend_params)


class HardFlatShader(_Shader):
    def forward(self, fragments, meshes, **kwargs):
        cameras, lights, materials, blend_params = self._parts(kwargs)
        texels = meshes.sample_textures(fragments)
        colors = flat_shading(meshes=meshes, fragments=fragments, texels=texels, lights=lights, cameras=cameras,
                              materials=materials, **self._view(kwargs))
        return hard_rgb_blend(colors, fragments, blend_params)
