"""pytorch3d.renderer.cameras (0.3.0): SfMOrthographicCameras and the look-at helpers, in torch (differentiable).

Row-vector convention as in PyTorch3D: world -> view is X R + T; SfMOrthographicCameras then maps
(x, y) -> (fx x + px, fy y + py) and keeps the view z."""
import math

import torch
import torch.nn.functional as Fn


def _batched(x, dim, device, dtype=torch.float32):
    t = torch.as_tensor(x, dtype=dtype, device=device) if not torch.is_tensor(x) else x.to(device)
    while t.dim() < dim:
        t = t[None]
    return t


class _WorldToView:
    """The world -> view transform (Transform3d's get_matrix / transform_points for one rotation + translation)."""

    def __init__(self, R, T):
        self.R, self.T = R, T

    def get_matrix(self):
        N = max(self.R.shape[0], self.T.shape[0])
        M = torch.zeros((N, 4, 4), dtype=self.R.dtype, device=self.R.device)
        M[:, :3, :3] = self.R
        M[:, 3, :3] = self.T
        M[:, 3, 3] = 1.0
        return M

    def transform_points(self, points):
        return torch.matmul(points, self.R) + self.T[:, None, :]


class SfMOrthographicCameras:
    def __init__(self, focal_length=1.0, principal_point=((0.0, 0.0),), R=None, T=None, device="cpu"):
        self.device = torch.device(device)
        self.R = _batched(torch.eye(3) if R is None else R, 3, self.device)
        self.T = _batched(torch.zeros(1, 3) if T is None else T, 2, self.device)
        fl = _batched(focal_length, 1, self.device)
        self.focal_length = fl[:, None].expand(-1, 2) if fl.dim() == 1 else fl
        self.principal_point = _batched(principal_point, 2, self.device)

    def __len__(self):
        return max(self.R.shape[0], self.T.shape[0])

    def to(self, device):
        return SfMOrthographicCameras(self.focal_length, self.principal_point, self.R, self.T, device)

    def get_world_to_view_transform(self, **kwargs):
        R = _batched(kwargs.get("R", self.R), 3, self.device)
        T = _batched(kwargs.get("T", self.T), 2, self.device)
        return _WorldToView(R, T)

    def get_camera_center(self, **kwargs):
        """-> [N,3] world position of the camera: C R + T = 0 (the specular term of phong_shading)."""
        w2v = self.get_world_to_view_transform(**kwargs)
        return -torch.matmul(w2v.T[:, None, :], torch.inverse(w2v.R))[:, 0]

    def transform_points(self, points, eps=None, **kwargs):
        """points [N,P,3] world -> (fx x_v + px, fy y_v + py, z_v) with (x_v, y_v, z_v) = X R + T."""
        del eps
        view = self.get_world_to_view_transform(**kwargs).transform_points(points)
        fl = _batched(kwargs.get("focal_length", self.focal_length), 1, self.device)
        if fl.dim() == 1:
            fl = fl[:, None].expand(-1, 2)
        pp = _batched(kwargs.get("principal_point", self.principal_point), 2, self.device)
        x = view[..., 0] * fl[:, None, 0] + pp[:, None, 0]
        y = view[..., 1] * fl[:, None, 1] + pp[:, None, 1]
        return torch.stack((x, y, view[..., 2]), dim=-1)


def look_at_rotation(camera_position, at=((0, 0, 0),), up=((0, 1, 0),), device="cpu"):
    cp = _batched(camera_position, 2, device)
    at = _batched(at, 2, device)
    up = _batched(up, 2, device)
    cp, at, up = torch.broadcast_tensors(cp, at, up)
    z_axis = Fn.normalize(at - cp, eps=1e-5)
    x_axis = Fn.normalize(torch.cross(up, z_axis, dim=1), eps=1e-5)
    y_axis = Fn.normalize(torch.cross(z_axis, x_axis, dim=1), eps=1e-5)
    is_close = torch.isclose(x_axis, torch.tensor(0.0, device=x_axis.device), atol=5e-3).all(dim=1, keepdim=True)
    if is_close.any():
        replacement = Fn.normalize(torch.cross(y_axis, z_axis, dim=1), eps=1e-5)
        x_axis = torch.where(is_close, replacement, x_axis)
    R = torch.cat((x_axis[:, None, :], y_axis[:, None, :], z_axis[:, None, :]), dim=1)
    return R.transpose(1, 2)


def camera_position_from_spherical_angles(distance, elevation, azimuth, degrees=True, device="cpu"):
    dist, elev, azim = (_batched(x, 1, device) for x in (distance, elevation, azimuth))
    if degrees:
        elev, azim = elev * (math.pi / 180.0), azim * (math.pi / 180.0)
    x = dist * torch.cos(elev) * torch.sin(azim)
    y = dist * torch.sin(elev)
    z = dist * torch.cos(elev) * torch.cos(azim)
    return torch.stack([x, y, z], dim=1).reshape(-1, 3)


def look_at_view_transform(dist=1.0, elev=0.0, azim=0.0, degrees=True, eye=None, at=((0, 0, 0),),
                           up=((0, 1, 0),), device="cpu"):
    """-> (R [N,3,3], T [N,3]) of a camera at `eye` (or at the spherical position dist / elev / azim) looking at `at`."""
    if eye is not None:
        C = _batched(eye, 2, device)
    else:
        C = camera_position_from_spherical_angles(dist, elev, azim, degrees=degrees, device=device)
        C = C + _batched(at, 2, device)
    R = look_at_rotation(C, at, up, device=device)
    T = -torch.bmm(R.transpose(1, 2), C[:, :, None])[:, :, 0]
    return R, T
