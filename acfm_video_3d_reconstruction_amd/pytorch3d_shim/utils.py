"""pytorch3d.utils.ico_sphere (utils/geometry.py:64; mesh_net.py builds its template sphere with it)."""
import functools

import numpy as np
import torch

from .ops import SubdivideMeshes
from .structures import Meshes


@functools.lru_cache(maxsize=None)
def _icosahedron():
    """The 12 vertices (0, +-1, +-phi) and their cyclic permutations on the unit sphere, and the 20 triples of mutual
    neighbours, each ordered so that its normal points away from the origin."""
    phi = (1.0 + 5.0 ** 0.5) / 2.0
    v = []
    for s1 in (-1.0, 1.0):
        for s2 in (-1.0, 1.0):
            v += [(0.0, s1, s2 * phi), (s1, s2 * phi, 0.0), (s2 * phi, 0.0, s1)]
    v = np.array(v)
    d2 = ((v[:, None] - v[None]) ** 2).sum(-1)
    near = np.abs(d2 - 4.0) < 1e-9                            # the edge length is 2
    faces = []
    for i in range(12):
        for j in range(i + 1, 12):
            for k in range(j + 1, 12):
                if near[i, j] and near[j, k] and near[i, k]:
                    out = np.dot(np.cross(v[j] - v[i], v[k] - v[i]), v[i] + v[j] + v[k]) > 0
                    faces.append((i, j, k) if out else (i, k, j))
    v = v / np.linalg.norm(v, axis=1, keepdims=True)
    return v.astype(np.float32), np.array(faces, np.int64)


@functools.lru_cache(maxsize=8)
def _ico_sphere_cpu(level):
    v, f = _icosahedron()
    mesh = Meshes(verts=[torch.from_numpy(v.copy())], faces=[torch.from_numpy(f.copy())])
    for _ in range(level):
        mesh = SubdivideMeshes()(mesh)
        v = mesh.verts_list()[0]
        mesh = Meshes(verts=[v / v.norm(dim=1, keepdim=True)], faces=mesh.faces_list())
    return mesh.verts_list()[0], mesh.faces_list()[0]


def ico_sphere(level: int = 0, device=None):
    """The unit icosahedron refined `level` times with SubdivideMeshes, every vertex put back on the unit sphere after
    each refinement: 10 * 4^level + 2 vertices, 20 * 4^level faces, closed (every edge in two faces), oriented
    outwards.  The ORDER of vertices and faces is this module's own: PyTorch3D's is not pinned."""
    if level < 0:
        raise ValueError("level must be >= 0")
    v, f = _ico_sphere_cpu(int(level))
    device = torch.device("cpu") if device is None else device
    return Meshes(verts=[v.clone().to(device)], faces=[f.clone().to(device)])
