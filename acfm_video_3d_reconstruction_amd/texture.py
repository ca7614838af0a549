"""The texture head's way from a UV image to the renderer's face atlas (multiframe/utils/mesh.py:191-232 and the
tail of TexturePredictorUV.forward, multiframe/nnutils/mesh_net.py:169-179).

    uv = compute_uvsampler(verts, faces[:num_faces], tex_size)          # once per model, numpy float64
    Hu, Wu = uv_image_size(num_faces, tex_size)
    atlas_of = UVAtlasSampler(torch.tensor(uv), symmetric=True, num_sym_faces=624)
    atlas = atlas_of(uvimage)                                           # [B,3,Hu,Wu] -> [B,F'+S,T,T,3]

On the GPU the module is ops.uv_atlas: one kernel forward, one backward, both reproducible to the bit."""
import threading

import numpy as np
import torch

from . import ops


def get_spherical_coords(X):
    """Points X [N,3] -> [N,2] = (u, v) in [-1, 1]: u from the azimuth atan2(y, x), v from the inclination
    acos(z / |X|), in float64 (utils/mesh.py:191-203)."""
    X = np.asarray(X, dtype=np.float64)
    theta = np.arccos(X[:, 2] / np.linalg.norm(X, axis=1))
    phi = np.arctan2(X[:, 1], X[:, 0])
    return np.stack([((phi + np.pi) / (2 * np.pi)) * 2 - 1, (theta / np.pi) * 2 - 1], 1)


def compute_uvsampler(verts, faces, tex_size=2):
    """UV coordinates of the tex_size x tex_size texels of every face: [F,T,T,2] float64 (utils/mesh.py:206-232).
    Texel (a, b) of a face (v0, v1, v2) is the point v2 + alpha_a (v0 - v2) + beta_b (v1 - v2) with
    alpha, beta = arange(T) / (T - 1), a the slower index; get_spherical_coords maps it to (u, v)."""
    T = int(tex_size)
    if T < 2:
        raise ValueError("tex_size must be at least 2 (texels sit at arange(T) / (T - 1)), got %d" % T)
    verts = np.asarray(verts, dtype=np.float64)
    steps = np.arange(T, dtype=np.float64) / (T - 1)
    ab = np.stack([np.repeat(steps, T), np.tile(steps, T)], 1)          # [T*T,2], alpha slower
    tri = verts[np.asarray(faces)]                                      # [F,3,3]
    v2 = tri[:, 2]
    edges = np.stack([tri[:, 0] - v2, tri[:, 1] - v2], 2)               # [F,3,2]
    pts = edges.dot(ab.T) + v2[:, :, None]                              # [F,3,T*T]
    uv = get_spherical_coords(pts.transpose(0, 2, 1).reshape(-1, 3))
    return uv.reshape(-1, T, T, 2)


def uv_image_size(num_faces, tex_size):
    """(Hu, Wu) of the UV image the texture network predicts for num_faces sampled faces (mesh_net.py:562-563)."""
    Hu = int(2 ** np.floor(np.log2(np.sqrt(num_faces) * tex_size)))
    return Hu, 2 * Hu


# one lock for every module's table cache: nn.DataParallel runs replicas (which share the cache of the module they
# were made from) on threads of their own
_LOCK = threading.RLock()


class UVAtlasSampler(torch.nn.Module):
    """uvimage [B,3,Hu,Wu] -> atlas [B,F'(+S),T,T,3], the lines mesh_net.py:169-179.

    uv_sampler: [F',T,T,2], or the reference's batched [B,F',T,T,2] of which row 0 is kept (mesh_net.py:155).  It is a
    constant of the model: kept as a float32 buffer outside the state dict (the reference keeps a plain attribute), and
    not to be written to afterwards -- the backward's table is built from it once per device and image size.
    symmetric=True appends the last num_sym_faces faces once more (1 <= num_sym_faces <= F'); symmetric=False ignores
    num_sym_faces (the reference passes -1 there)."""

    def __init__(self, uv_sampler, symmetric=False, num_sym_faces=None):
        super().__init__()
        s = torch.as_tensor(uv_sampler)
        if s.dim() == 5:
            s = s[0]
        if s.dim() != 4 or s.shape[1] != s.shape[2] or s.shape[3] != 2 or s.shape[0] < 1 or s.shape[1] < 1:
            raise ValueError("uv_sampler: [F',T,T,2] or [B,F',T,T,2] expected, got %s" % (tuple(uv_sampler.shape),))
        self.symmetric = bool(symmetric)
        self.num_faces, self.tex_size = int(s.shape[0]), int(s.shape[1])
        if self.symmetric:
            if num_sym_faces is None or not 1 <= int(num_sym_faces) <= self.num_faces:
                # (the reference's tex_pred[:, -0:] would silently append EVERY face)
                raise ValueError("num_sym_faces must lie in [1, F'] = [1, %d] with symmetric=True, got %r"
                                 % (self.num_faces, num_sym_faces))
            self.num_sym_faces = int(num_sym_faces)
        else:
            self.num_sym_faces = 0
        self.register_buffer("uv_sampler", s.detach().to(torch.float32).contiguous().clone(), persistent=False)
        self._tables = {}        # (device, Hu, Wu) -> ops.UVAtlasTable; shared with DataParallel replicas

    def table(self, device, Hu, Wu):
        """The ops.UVAtlasTable for this device and image size, built on first use (never inside a graph capture: run
        the module, or this, once before capturing)."""
        key = (str(device), int(Hu), int(Wu))
        with _LOCK:
            t = self._tables.get(key)
            if t is None:
                t = self._tables[key] = ops.uv_atlas_table(self.uv_sampler, Hu, Wu)
            return t

    def forward(self, uvimage):
        if uvimage.dim() != 4:
            raise ValueError("uvimage: [B,3,Hu,Wu] expected, got %s" % (tuple(uvimage.shape),))
        if uvimage.device != self.uv_sampler.device:
            raise ValueError("uvimage is on %s, the module on %s" % (uvimage.device, self.uv_sampler.device))
        return ops.uv_atlas(uvimage, self.table(uvimage.device, uvimage.shape[2], uvimage.shape[3]), self.num_sym_faces)
