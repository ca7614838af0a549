"""The reference's mesh viewer (multiframe/utils/bird_vis.py:15-158, VisRenderer), written from its behaviour:
uint8 views of a predicted shape from the predicted camera, a rotated shape or another viewpoint, in the default
light-blue vertex colour or with a texture.

Unlit, a call is the NeuralRenderer texture render, clipped and scaled.  set_light_dir -- an empty body in the
reference, so its untextured views are flat silhouettes -- does what its signature says here: the render then goes
through the shim's MeshRenderer with the reference's view (nmr.py:144-149), DirectionalLights(ambient = int_amb,
diffuse = int_dir, specular = 0, direction) and SoftPhongShader, i.e. the lit kernels of ops.phong_shade.

The rotation helpers (Rodrigues' formula, rotation matrix to quaternion) are numpy; there is no cv2 here.
Keypoint drawing (kp2im) is out of scope: diff_vp(kp_verts=...) returns (image, projected keypoints)."""
import numpy as np
import torch

from . import ops
from .nnutils.nmr import NeuralRenderer

DEFAULT_COLOUR = (156.0 / 255.0, 199.0 / 255.0, 234.0 / 255.0)


def rodrigues(rvec):
    """Rotation vector (axis times angle in radians) -> 3 x 3 rotation matrix: I + sin(t) K + (1 - cos(t)) K^2."""
    r = np.asarray(rvec, dtype=np.float64).reshape(3)
    theta = float(np.linalg.norm(r))
    if theta < 1e-12:
        return np.eye(3)
    k = r / theta
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(theta) * K + (1.0 - np.cos(theta)) * (K @ K)


def quaternion_from_matrix(R):
    """Rotation matrix (3 x 3, or the upper left of a 4 x 4) -> unit quaternion (w, x, y, z), w >= 0: the branch with
    the largest of (trace, R00, R11, R22) under the root, so no division by a small number."""
    R = np.asarray(R, dtype=np.float64)[:3, :3]
    t = np.trace(R)
    if t > 0.0:
        s = 2.0 * np.sqrt(1.0 + t)
        q = np.array([0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s])
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = 2.0 * np.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k])
        q = np.zeros(4)
        q[0] = (R[k, j] - R[j, k]) / s
        q[1 + i] = 0.25 * s
        q[1 + j] = (R[j, i] + R[i, j]) / s
        q[1 + k] = (R[k, i] + R[i, k]) / s
    q = q / np.linalg.norm(q)
    return -q if q[0] < 0.0 else q


def quaternion_matrix(q):
    """Unit quaternion (w, x, y, z) -> 3 x 3 rotation matrix."""
    w, x, y, z = np.asarray(q, dtype=np.float64).reshape(4) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def default_camera():
    """(scale 0.75, no translation, the side view): a third of a turn about x, then a quarter about y."""
    R = rodrigues([0.0, np.pi / 2, 0.0]) @ rodrigues([np.pi / 3, 0.0, 0.0])
    return np.concatenate([[0.75, 0.0, 0.0], quaternion_from_matrix(R)]).astype(np.float32)


def viewpoint_camera(cam, angle=90, axis=(1, 0, 0), new_ext=None, extra_elev=False):
    """The 7-vector camera of diff_vp: the rotation of `cam` turned by `angle` degrees about `axis` (rotate_by . R),
    a further 20 degrees of elevation about x if asked, behind the extrinsics new_ext (scale, tx, ty; 0.6, 0, 0)."""
    cam = np.asarray(cam, dtype=np.float64).reshape(-1)
    R = rodrigues(np.deg2rad(angle) * np.asarray(axis, dtype=np.float64)) @ quaternion_matrix(cam[-4:])
    if extra_elev:
        R = rodrigues([np.pi / 9, 0.0, 0.0]) @ R
    ext = [0.6, 0.0, 0.0] if new_ext is None else list(new_ext)
    return np.concatenate([ext, quaternion_from_matrix(R)]).astype(np.float32)


class VisRenderer:
    """VisRenderer(img_size, faces): faces [F,3] or [1,F,3] (array or tensor).  Views are uint8 [H,W,3]."""

    def __init__(self, img_size, faces, device="cuda"):
        self.img_size = int(img_size)
        self.device = torch.device(device)
        self.renderer = NeuralRenderer(self.img_size)
        f = torch.as_tensor(np.asarray(faces.cpu() if torch.is_tensor(faces) else faces)).to(torch.int64)
        self.faces = (f[None] if f.dim() == 2 else f).to(self.device)
        self.default_cam = torch.from_numpy(default_camera()).to(self.device)[None]
        self.light = None

    def set_bgcolor(self, color):
        self.renderer.set_bgcolor(color)

    def set_light_dir(self, direction, int_dir=0.8, int_amb=0.8):
        """A directional light of intensity int_dir from `direction` over an ambient light of intensity int_amb;
        direction=None switches the lighting off again."""
        if direction is None:
            self.light = None
            return
        d = [float(x) for x in np.asarray(direction, dtype=np.float64).reshape(3)]
        self.light = (d, float(int_dir), float(int_amb))

    def _lit(self, verts, cams, texture, atlas):
        from .pytorch3d_shim.renderer import (BlendParams, DirectionalLights, MeshRasterizer, MeshRenderer,
                                              RasterizationSettings, SfMOrthographicCameras, SoftPhongShader,
                                              Textures, TexturesAtlas, look_at_view_transform)
        from .pytorch3d_shim.structures import Meshes
        direction, int_dir, int_amb = self.light
        dev = verts.device
        vs = ops.project(verts, cams) * torch.tensor([1.0, -1.0, 1.0], device=dev)
        R, T = look_at_view_transform(eye=((0, 0, -2.732),), device=dev)
        R[:, 0, 0] *= -1
        cameras = SfMOrthographicCameras(device=dev)
        lights = DirectionalLights(ambient_color=((int_amb,) * 3,), diffuse_color=((int_dir,) * 3,),
                                   specular_color=((0.0, 0.0, 0.0),), direction=(tuple(direction),), device=dev)
        renderer = MeshRenderer(
            rasterizer=MeshRasterizer(cameras=cameras, raster_settings=RasterizationSettings(
                image_size=self.img_size, blur_radius=0.0, faces_per_pixel=1, clip_barycentric_coords=True)),
            shader=SoftPhongShader(device=dev, cameras=cameras, lights=lights,
                                   blend_params=BlendParams(background_color=0)))
        tex = TexturesAtlas(atlas=texture) if atlas else Textures(verts_rgb=texture)
        mesh = Meshes(verts=vs, faces=self.faces.expand(vs.shape[0], -1, -1), textures=tex)
        return renderer(meshes_world=mesh, R=R.to(dev), T=T.to(dev))[..., :3].permute(0, 3, 1, 2)

    @torch.no_grad()
    def __call__(self, verts, cams=None, texture=None, atlas=True):
        """verts [V,3] (or [1,V,3]), cams [7] (default: the side view), texture: None (the default colour on every
        vertex), vertex colours [V,3] with atlas=False, or a face atlas [F,R,R,3] -> uint8 [H,W,3]."""
        verts = torch.as_tensor(verts, dtype=torch.float32).to(self.device)
        verts = verts[None] if verts.dim() == 2 else verts
        cams = self.default_cam if cams is None else torch.as_tensor(cams, dtype=torch.float32).to(self.device)
        cams = cams[None] if cams.dim() == 1 else cams
        if texture is None:
            texture = torch.tensor(DEFAULT_COLOUR, device=self.device).expand(1, verts.shape[1], 3).contiguous()
            atlas = False
        else:
            texture = torch.as_tensor(texture, dtype=torch.float32).to(self.device)
            if texture.dim() == (4 if atlas else 2):
                texture = texture[None]
        if self.light is None:
            rend = self.renderer.forward(verts, self.faces, cams, texture, atlas=atlas)[0]
        else:
            rend = self._lit(verts, cams, texture, atlas)
        rend = rend[0].permute(1, 2, 0).clamp(0.0, 1.0) * 255.0
        return rend.cpu().numpy().astype(np.uint8)

    def rotated(self, vert, deg, axis=(0, 1, 0), cam=None, texture=None, atlas=True):
        """The shape turned by `deg` degrees about `axis` through its own centre, seen from `cam`."""
        vert = torch.as_tensor(vert, dtype=torch.float32).to(self.device)
        rot = torch.from_numpy(rodrigues(np.deg2rad(deg) * np.asarray(axis, dtype=np.float64))).to(vert)
        centre = vert.mean(0)
        return self(torch.matmul(vert - centre, rot.t()) + centre, cams=cam, texture=texture, atlas=atlas)

    def diff_vp(self, verts, cam=None, angle=90, axis=(1, 0, 0), texture=None, kp_verts=None, new_ext=None,
                extra_elev=False, atlas=True):
        """The shape from another viewpoint (viewpoint_camera).  With kp_verts [K,3] -> (image, their projections
        [K,2] in that view) instead of the image alone."""
        cam = self.default_cam[0] if cam is None else torch.as_tensor(cam)
        new_cam = torch.from_numpy(viewpoint_camera(cam.detach().cpu().numpy(), angle, axis, new_ext, extra_elev))
        new_cam = new_cam.to(self.device)
        img = self(verts, cams=new_cam, texture=texture, atlas=atlas)
        if kp_verts is None:
            return img
        kp = torch.as_tensor(kp_verts, dtype=torch.float32).to(self.device)
        kps = self.renderer.project_points(kp[None], new_cam[None])
        return img, kps[0].detach().cpu().numpy()
