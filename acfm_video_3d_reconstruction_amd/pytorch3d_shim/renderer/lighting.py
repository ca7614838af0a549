"""pytorch3d.renderer.lighting (0.3.0): DirectionalLights, PointLights and the diffuse / specular terms, in torch.
Colours, directions and locations are [N or 1, 3]; they broadcast per mesh over the [N, ..., 3] points and normals."""
import torch
import torch.nn.functional as Fn


def _prop(x, device):
    t = x.to(device=device, dtype=torch.float32) if torch.is_tensor(x) else torch.tensor(x, dtype=torch.float32,
                                                                                         device=device)
    return t.reshape(-1, 3)


def _per_mesh(t, like):
    """[N or 1, 3] -> [N or 1, 1, ..., 1, 3] against like [N, ..., 3]."""
    return t.reshape((t.shape[0],) + (1,) * (like.dim() - 2) + (3,))


def diffuse(normals, color, direction):
    """color * relu(n . l), n and l normalised with eps 1e-6; direction [N,3] or per point."""
    if direction.shape != normals.shape:
        direction = _per_mesh(direction, normals)
    normals = Fn.normalize(normals, p=2, dim=-1, eps=1e-6)
    direction = Fn.normalize(direction, p=2, dim=-1, eps=1e-6)
    angle = Fn.relu(torch.sum(normals * direction, dim=-1))
    return _per_mesh(color, normals) * angle[..., None]


def specular(points, normals, direction, color, camera_position, shininess):
    """color * relu(v . r)^shininess [n . l > 0], r = 2 (n . l) n - l, v = normalise(camera_position - points)."""
    if direction.shape != normals.shape:
        direction = _per_mesh(direction, normals)
    normals = Fn.normalize(normals, p=2, dim=-1, eps=1e-6)
    direction = Fn.normalize(direction, p=2, dim=-1, eps=1e-6)
    cos_angle = torch.sum(normals * direction, dim=-1)
    mask = (cos_angle > 0).to(torch.float32)
    view_direction = Fn.normalize(_per_mesh(camera_position, points) - points, p=2, dim=-1, eps=1e-6)
    reflect_direction = -direction + 2 * (cos_angle[..., None] * normals)
    alpha = Fn.relu(torch.sum(view_direction * reflect_direction, dim=-1)) * mask
    shininess = shininess.reshape((-1,) + (1,) * (alpha.dim() - 1)) if torch.is_tensor(shininess) else shininess
    return _per_mesh(color, normals) * torch.pow(alpha, shininess)[..., None]


class _Lights:
    _fields = ("ambient_color", "diffuse_color", "specular_color")

    def __init__(self, device="cpu", **props):
        self.device = torch.device(device)
        for k, v in props.items():
            setattr(self, k, _prop(v, self.device))

    def _props(self):
        return {k: getattr(self, k) for k in self._fields}

    def clone(self):
        return type(self)(device=self.device, **{k: v.clone() for k, v in self._props().items()})

    def to(self, device):
        self.device = torch.device(device)
        for k, v in self._props().items():
            setattr(self, k, v.to(self.device))
        return self

    def no_diffuse_or_specular(self):
        """True when the diffuse and specular colours are all zero: the light is ambient only."""
        return bool((self.diffuse_color == 0).all()) and bool((self.specular_color == 0).all())


class DirectionalLights(_Lights):
    _fields = _Lights._fields + ("direction",)

    def __init__(self, ambient_color=((0.5, 0.5, 0.5),), diffuse_color=((0.3, 0.3, 0.3),),
                 specular_color=((0.2, 0.2, 0.2),), direction=((0, 1, 0),), device="cpu"):
        super().__init__(device, ambient_color=ambient_color, diffuse_color=diffuse_color,
                         specular_color=specular_color, direction=direction)

    def diffuse(self, normals, points=None):
        return diffuse(normals=normals, color=self.diffuse_color, direction=self.direction)

    def specular(self, normals, points, camera_position, shininess):
        return specular(points=points, normals=normals, color=self.specular_color, direction=self.direction,
                        camera_position=camera_position, shininess=shininess)


class PointLights(_Lights):
    _fields = _Lights._fields + ("location",)

    def __init__(self, ambient_color=((0.5, 0.5, 0.5),), diffuse_color=((0.3, 0.3, 0.3),),
                 specular_color=((0.2, 0.2, 0.2),), location=((0, 1, 0),), device="cpu"):
        super().__init__(device, ambient_color=ambient_color, diffuse_color=diffuse_color,
                         specular_color=specular_color, location=location)

    def diffuse(self, normals, points):
        return diffuse(normals=normals, color=self.diffuse_color, direction=_per_mesh(self.location, points) - points)

    def specular(self, normals, points, camera_position, shininess):
        return specular(points=points, normals=normals, color=self.specular_color,
                        direction=_per_mesh(self.location, points) - points, camera_position=camera_position,
                        shininess=shininess)
