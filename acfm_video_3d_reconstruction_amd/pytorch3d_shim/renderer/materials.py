"""pytorch3d.renderer.materials (0.3.0): Materials (ambient / diffuse / specular reflectance, shininess)."""
import torch

from .lighting import _prop


class Materials:
    def __init__(self, ambient_color=((1, 1, 1),), diffuse_color=((1, 1, 1),), specular_color=((1, 1, 1),),
                 shininess=64, device="cpu"):
        self.device = torch.device(device)
        self.ambient_color = _prop(ambient_color, self.device)
        self.diffuse_color = _prop(diffuse_color, self.device)
        self.specular_color = _prop(specular_color, self.device)
        self.shininess = shininess

    def clone(self):
        return Materials(self.ambient_color.clone(), self.diffuse_color.clone(), self.specular_color.clone(),
                         self.shininess, self.device)

    def to(self, device):
        self.device = torch.device(device)
        for k in ("ambient_color", "diffuse_color", "specular_color"):
            setattr(self, k, getattr(self, k).to(self.device))
        return self
