"""pytorch3d.renderer.mesh.rasterizer (0.3.0): Fragments, RasterizationSettings, MeshRasterizer."""
from typing import NamedTuple, Optional

import torch
from torch import nn

from .rasterize_meshes import check_raster_options, rasterize_meshes


class Fragments(NamedTuple):
    pix_to_face: torch.Tensor
    zbuf: torch.Tensor
    bary_coords: torch.Tensor
    dists: Optional[torch.Tensor]


class RasterizationSettings:
    __slots__ = ["image_size", "blur_radius", "faces_per_pixel", "bin_size", "max_faces_per_bin",
                 "perspective_correct", "clip_barycentric_coords", "cull_backfaces"]

    def __init__(self, image_size=256, blur_radius=0.0, faces_per_pixel=1, bin_size=None, max_faces_per_bin=None,
                 perspective_correct=False, clip_barycentric_coords=False, cull_backfaces=False):
        # what the HIP rasterizer cannot do is refused here already, by name (bin_size / max_faces_per_bin: ignored)
        check_raster_options(image_size, faces_per_pixel, perspective_correct, cull_backfaces)
        self.image_size = image_size
        self.blur_radius = blur_radius
        self.faces_per_pixel = faces_per_pixel
        self.bin_size = bin_size
        self.max_faces_per_bin = max_faces_per_bin
        self.perspective_correct = perspective_correct
        self.clip_barycentric_coords = clip_barycentric_coords
        self.cull_backfaces = cull_backfaces


class MeshRasterizer(nn.Module):
    """Meshes in world coordinates -> Fragments.  `forward(meshes_world, **kwargs)`: kwargs may override the
    camera (`cameras=`) and its `R=` / `T=` (as the reference's NeuralRenderer.rasterize_of does)."""

    def __init__(self, cameras=None, raster_settings=None):
        super().__init__()
        self.cameras = cameras
        self.raster_settings = raster_settings if raster_settings is not None else RasterizationSettings()

    def transform(self, meshes_world, **kwargs):
        cameras = kwargs.get("cameras", self.cameras)
        if cameras is None:
            raise ValueError("Cameras must be specified either at initialization or in the forward pass of "
                             "MeshRasterizer")
        verts_screen = cameras.transform_points(meshes_world.verts_padded(), **kwargs)
        return meshes_world.update_padded(new_verts_padded=verts_screen)

    def to(self, device):
        if self.cameras is not None:
            self.cameras = self.cameras.to(device)
        return self

    def forward(self, meshes_world, **kwargs):
        meshes_screen = self.transform(meshes_world, **kwargs)
        rs = kwargs.get("raster_settings", self.raster_settings)
        pix_to_face, zbuf, bary_coords, dists = rasterize_meshes(
            meshes_screen, image_size=rs.image_size, blur_radius=rs.blur_radius, faces_per_pixel=rs.faces_per_pixel,
            bin_size=rs.bin_size, max_faces_per_bin=rs.max_faces_per_bin, perspective_correct=rs.perspective_correct,
            clip_barycentric_coords=rs.clip_barycentric_coords, cull_backfaces=rs.cull_backfaces)
        return Fragments(pix_to_face=pix_to_face, zbuf=zbuf, bary_coords=bary_coords, dists=dists)
