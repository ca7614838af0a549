"""pytorch3d.ops.SubdivideMeshes (multiframe/main.py:196-199; semantics: SURVEY App-A.8) and
interpolate_face_attributes (the HIP kernel of ops.interpolate_face_attributes); sample_points_from_meshes as
utils/geometry.py:111-112 calls it."""
import torch

from ..ops import interpolate_face_attributes  # noqa: F401  (pytorch3d.ops.interpolate_face_attributes)
from .structures import Meshes


class SubdivideMeshes(torch.nn.Module):
    """One 1->4 subdivision: a new vertex at every edge midpoint (appended after the originals
    in edges_packed order); face (v0,v1,v2) with edge ids e0=v1v2, e1=v0v2, e2=v0v1 becomes
    (v0,e2,e1), (v1,e0,e2), (v2,e1,e0), (e0,e1,e2), concatenated as [all f0; f1; f2; f3]."""

    def __init__(self, meshes=None):
        super().__init__()
        self.precomputed = False
        if meshes is not None:
            if len(meshes) != 1:
                raise ValueError("Mesh can only have one mesh.")
            self.register_buffer("_subdivided_faces", self._subdivide_faces(meshes))
            self.precomputed = True

    @staticmethod
    def _subdivide_faces(mesh):
        faces = mesh.faces_packed()
        edges = mesh.edges_packed()
        V = mesh.verts_packed().shape[0]
        key = edges[:, 0] * V + edges[:, 1]

        def eid(a, b):
            k = torch.minimum(a, b) * V + torch.maximum(a, b)
            return torch.searchsorted(key, k) + V

        v0, v1, v2 = faces[:, 0], faces[:, 1], faces[:, 2]
        e0, e1, e2 = eid(v1, v2), eid(v0, v2), eid(v0, v1)
        f0 = torch.stack([v0, e2, e1], 1)
        f1 = torch.stack([v1, e0, e2], 1)
        f2 = torch.stack([v2, e1, e0], 1)
        f3 = torch.stack([e0, e1, e2], 1)
        return torch.cat([f0, f1, f2, f3], 0)

    def forward(self, meshes, feats=None):
        if feats is not None:
            raise NotImplementedError("per-vertex features are not used by the reference")
        out_v, out_f = [], []
        for i in range(len(meshes)):
            m = Meshes(verts=[meshes.verts_list()[i]], faces=[meshes.faces_list()[i]])
            faces = self._subdivided_faces if self.precomputed else self._subdivide_faces(m)
            e = m.edges_packed()
            v = m.verts_packed()
            out_v.append(torch.cat([v, 0.5 * (v[e[:, 0]] + v[e[:, 1]])], 0))
            out_f.append(faces)
        return Meshes(verts=out_v, faces=out_f)


def sample_points_from_faces(verts, faces, face_idx, u, v, return_normals=False):
    """The deterministic half of sample_points_from_meshes: verts [P,3], faces [F,3] (packed ids), face_idx [N,S] rows
    of `faces`, u, v [N,S] in [0,1) -> points [N,S,3] = w0 v0 + w1 v1 + w2 v2 with w0 = 1 - sqrt(u),
    w1 = sqrt(u) (1 - v), w2 = sqrt(u) v: uniform over each triangle.  Differentiable in verts.  With return_normals
    also the unit normals (v1 - v0) x (v2 - v0) / |.| of those faces."""
    tri = verts[faces.long()[face_idx]]                      # [N,S,3,3]
    a, b, c = tri[:, :, 0], tri[:, :, 1], tri[:, :, 2]
    su = u.sqrt()
    w0, w1, w2 = 1.0 - su, su * (1.0 - v), su * v
    points = w0[..., None] * a + w1[..., None] * b + w2[..., None] * c
    if not return_normals:
        return points
    n = torch.cross(b - a, c - a, dim=2)
    return points, n / n.norm(dim=2, p=2, keepdim=True).clamp(min=1e-12)


def sample_points_from_meshes(meshes, num_samples: int = 10000, return_normals: bool = False):
    """PyTorch3D 0.3.0's sampling: per mesh, num_samples faces drawn with replacement with probability proportional to
    their area (0.5 |(v1 - v0) x (v2 - v0)|, no gradient), then a uniform point of each (sample_points_from_faces).
    -> [N, num_samples, 3] (and the faces' unit normals); a mesh without faces yields zeros.  The draws are
    torch.multinomial and torch.rand on the meshes' device: the same distribution as PyTorch3D's, not its random
    stream."""
    if meshes.isempty():
        raise ValueError("Meshes are empty.")
    verts, faces = meshes.verts_packed(), meshes.faces_packed()
    N, dev = len(meshes), verts.device
    with torch.no_grad():
        fv = verts.detach()[faces]
        areas = 0.5 * torch.cross(fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0], dim=1).norm(dim=1)
        counts = [f.shape[0] for f in meshes.faces_list()]
        idx = torch.zeros((N, num_samples), dtype=torch.int64, device=dev)
        first = 0
        for i, n in enumerate(counts):
            if n > 0:
                idx[i] = torch.multinomial(areas[first:first + n], num_samples, replacement=True) + first
            first += n
    u, v = torch.rand(N, num_samples, dtype=verts.dtype, device=dev), torch.rand(N, num_samples, dtype=verts.dtype, device=dev)
    if faces.shape[0] == 0:
        z = verts.new_zeros((N, num_samples, 3))
        return (z, z.clone()) if return_normals else z
    out = sample_points_from_faces(verts, faces, idx, u, v, return_normals)
    if all(n > 0 for n in counts):
        return out
    live = torch.tensor([n > 0 for n in counts], device=dev)[:, None, None]
    if return_normals:
        return torch.where(live, out[0], torch.zeros_like(out[0])), torch.where(live, out[1], torch.zeros_like(out[1]))
    return torch.where(live, out, torch.zeros_like(out))
