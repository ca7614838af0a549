"""pytorch3d.ops.SubdivideMeshes (multiframe/main.py:196-199; semantics: SURVEY App-A.8) and
interpolate_face_attributes (the HIP kernel of ops.interpolate_face_attributes); sample_points_from_meshes as
utils/geometry.py:111-112 calls it; knn_points / knn_gather, PyTorch3D 0.3.0's point-set pair (the kernels of
csrc/acfm_knn.hip for GPU tensors, the same definition in torch ops for host tensors)."""
import collections
import contextlib

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


_DEFAULT_SAMPLER = [None]     # what default_sampler() installs: used by calls that pass no sampler


@contextlib.contextmanager
def default_sampler(sampler):
    """with default_sampler(SurfaceSampler(seed)): ...   -- inside the block sample_points_from_meshes calls that pass
    no sampler use this one, so code that cannot be edited (the reference's fit_verts_to_mesh) draws on the kernel.
    Off by default; process-wide while the block runs."""
    prev = _DEFAULT_SAMPLER[0]
    _DEFAULT_SAMPLER[0] = sampler
    try:
        yield sampler
    finally:
        _DEFAULT_SAMPLER[0] = prev


class _HostSurfacePoints(torch.autograd.Function):
    """The definition's own points (numpy, bit for bit) as a function of the vertices: the gradient of vertex k of a
    sample's face is its weight w_k, as in ops.sample_surface's backward."""

    @staticmethod
    def forward(ctx, verts, ids, w, points):
        ctx.save_for_backward(ids, w)
        ctx.P = verts.shape[0]
        return points.to(verts.dtype)

    @staticmethod
    def backward(ctx, g):
        ids, w = ctx.saved_tensors                                   # [N,S,3] each
        gv = g.new_zeros((ctx.P, 3))
        gv.index_add_(0, ids.reshape(-1), (w[..., None].to(g.dtype) * g[:, :, None, :]).reshape(-1, 3))
        return gv, None, None, None


def _sample_with(sampler, meshes, num_samples, return_normals):
    """The counter-based draw of surface_sampling: the kernel for GPU tensors, the numpy definition for host tensors;
    the point (host) and the normals are the torch lines of sample_points_from_faces on the drawn faces."""
    verts, faces = meshes.verts_packed(), meshes.faces_packed()
    counts = [f.shape[0] for f in meshes.faces_list()]
    first = [0]
    for n in counts:
        first.append(first[-1] + n)
    N, S = len(meshes), int(num_samples)
    if verts.is_cuda:
        from .. import ops
        sizes = {v.shape[0] for v in meshes.verts_list()}
        vpm = sizes.pop() if len(sizes) == 1 else 0
        points, fidx = ops.sample_surface(sampler.state_on(verts.device), verts, faces,
                                          torch.tensor(first, dtype=torch.int64), S, verts_per_mesh=vpm)
        if not return_normals:
            return points
        live = fidx >= 0
    else:
        pts, fi, uv = sampler.draw_host(verts.detach().numpy(), faces.numpy(), first, S)
        fidx, uv = torch.from_numpy(fi), torch.from_numpy(uv)
        live = fidx >= 0
        if faces.shape[0] == 0:
            points = verts.new_zeros((N, S, 3))
        else:
            su = uv[..., 0].sqrt()
            w = torch.stack([1.0 - su, su * (1.0 - uv[..., 1]), su * uv[..., 1]], -1) * live[..., None]
            points = _HostSurfacePoints.apply(verts, faces.long()[fidx.long().clamp(min=0)], w, torch.from_numpy(pts))
        if not return_normals:
            return points
    if faces.shape[0] == 0:
        return points, torch.zeros_like(points)
    tri = verts[faces.long()[fidx.long().clamp(min=0)]]
    a, b, c = tri[:, :, 0], tri[:, :, 1], tri[:, :, 2]
    n = torch.cross(b - a, c - a, dim=2)
    n = n / n.norm(dim=2, p=2, keepdim=True).clamp(min=1e-12)
    return points, torch.where(live[..., None], n, torch.zeros_like(n))


def sample_points_from_meshes(meshes, num_samples: int = 10000, return_normals: bool = False, sampler=None):
    """PyTorch3D 0.3.0's sampling: per mesh, num_samples faces drawn with replacement with probability proportional to
    their area (0.5 |(v1 - v0) x (v2 - v0)|, no gradient), then a uniform point of each (sample_points_from_faces).
    -> [N, num_samples, 3] (and the faces' unit normals); a mesh without faces yields zeros.  The draws are
    torch.multinomial and torch.rand on the meshes' device: the same distribution as PyTorch3D's, not its random
    stream.
    sampler (a surface_sampling.SurfaceSampler, or the one default_sampler() installed): the draws are that module's
    counter-based ones instead -- ops.sample_surface on the GPU, its numpy definition on host tensors -- which a
    hipGraph can contain and a test can predict; areas are then quantised to 24 bits of the mesh's largest face."""
    if meshes.isempty():
        raise ValueError("Meshes are empty.")
    if sampler is None:
        sampler = _DEFAULT_SAMPLER[0]
    if sampler is not None:
        return _sample_with(sampler, meshes, num_samples, return_normals)
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


# ------------------------------------------------------------------------------------------ knn_points, knn_gather
_KNN = collections.namedtuple("KNN", "dists idx knn")


def _sq_dist(e):
    """Sum of squares over the last dimension, left to right: (dx dx + dy dy) + dz dz for D = 3, as the kernels."""
    acc = e[..., 0] * e[..., 0]
    for k in range(1, e.shape[-1]):
        acc = acc + e[..., k] * e[..., k]
    return acc


def _knn_points_host(p1, p2, l1, l2, K):
    """The definition of ops.knn_points in torch ops, any D: the K nearest are chosen under no_grad (numpy's stable
    argsort: the lower index first among equal distances), the distances to them are recomputed differentiably."""
    N, P1, _ = p1.shape
    P2 = p2.shape[1]
    with torch.no_grad():
        d = _sq_dist(p1[:, :, None, :] - p2[:, None, :, :])                       # [N,P1,P2]
        v1 = torch.arange(P1)[None] < l1[:, None]                                 # [N,P1] rows that count
        v2 = torch.arange(P2)[None] < l2[:, None]
        d = torch.where(v1[:, :, None] & v2[:, None, :], d, torch.full_like(d, float("inf")))   # (padding may hold NaN)
        order = torch.from_numpy(d.numpy().argsort(axis=2, kind="stable"))[:, :, :K]
        idx = torch.zeros((N, P1, K), dtype=torch.int64)
        idx[:, :, :order.shape[2]] = order
        valid = v1[:, :, None] & (torch.arange(K)[None, None, :] < l2.clamp(max=K)[:, None, None])
        idx = torch.where(valid, idx, torch.zeros_like(idx))
    zero = torch.zeros((), dtype=p1.dtype)
    near = p2[:, :, None, :].expand(N, P2, K, p2.shape[2]).gather(1, idx[..., None].expand(N, P1, K, p2.shape[2]))
    e = torch.where(valid[..., None], p1[:, :, None, :], zero) - torch.where(valid[..., None], near, zero)
    return _sq_dist(e), idx


def knn_points(p1, p2, lengths1=None, lengths2=None, K: int = 1, version: int = -1, return_nn: bool = False,
               return_sorted: bool = True):
    """pytorch3d.ops.knn_points -> the namedtuple (dists [N,P1,K], idx [N,P1,K] int64, knn [N,P1,K,D] or None).  For
    every point of p1[n, :lengths1[n]] its min(K, lengths2[n]) nearest points of p2[n, :lengths2[n]]: squared distances,
    ascending, the lower index first among equal distances; every other slot holds 0 / 0 (PyTorch3D's padding).  Rows
    at or past a length are never used (they may hold NaN).  knn = knn_gather(p2, idx, lengths2) when return_nn.
    `version` is accepted and ignored; return_sorted=False returns the same sorted lists (PyTorch3D leaves that order
    open).  GPU tensors run ops.knn_points (float32, D = 3, K <= 32; the gradient of p2 is summed with float atomics
    and is not bit-reproducible); host tensors run the same definition in torch ops with any D and K."""
    if not torch.is_tensor(p1) or not torch.is_tensor(p2) or p1.dim() != 3 or p2.dim() != 3:
        raise ValueError("knn_points: p1 [N,P1,D] and p2 [N,P2,D] tensors expected")
    if p1.shape[0] != p2.shape[0]:
        raise ValueError("pts1 and pts2 must have the same batch dimension.")
    if p1.shape[2] != p2.shape[2]:
        raise ValueError("pts1 and pts2 must have the same point dimension.")
    N, P1, P2 = p1.shape[0], p1.shape[1], p2.shape[1]
    for name, t in (("lengths1", lengths1), ("lengths2", lengths2)):
        if t is not None and tuple(t.shape) != (N,):
            raise ValueError("knn_points: %s must have shape (N,) = (%d,)" % (name, N))
    if p1.is_cuda:
        from .. import ops
        dists, idx = ops.knn_points(p1, p2, lengths1, lengths2, K)
    else:
        if int(K) != K or K < 1:
            raise ValueError("knn_points: K must be at least 1, got %r" % (K,))
        if N == 0 or P1 == 0 or P2 == 0:
            raise ValueError("knn_points: p1 and p2 must hold at least one cloud of at least one point each")
        l1 = torch.full((N,), P1, dtype=torch.int64) if lengths1 is None else lengths1.long().clamp(0, P1)
        l2 = torch.full((N,), P2, dtype=torch.int64) if lengths2 is None else lengths2.long().clamp(0, P2)
        dists, idx = _knn_points_host(p1, p2, l1, l2, int(K))
    return _KNN(dists, idx, knn_gather(p2, idx, lengths2) if return_nn else None)


def knn_gather(x, idx, lengths=None):
    """pytorch3d.ops.knn_gather: x [N,M,U], idx [N,L,K], lengths [N] of x's clouds or None -> [N,L,K,U] with
    out[n,l,k] = x[n, idx[n,l,k]], and zeros where k >= lengths[n].  On the GPU (ops.knn_gather) an index outside
    [0, M) is not dereferenced and yields zeros; on the host it raises as torch.gather does."""
    if x.dim() != 3 or idx.dim() != 3 or x.shape[0] != idx.shape[0]:
        raise ValueError("knn_gather: x [N,M,U] and idx [N,L,K] expected, got %s and %s" % (tuple(x.shape), tuple(idx.shape)))
    N, M, U = x.shape
    _, L, K = idx.shape
    if lengths is not None and tuple(lengths.shape) != (N,):
        raise ValueError("x and lengths must have same batch dimension.")
    if x.is_cuda:
        from .. import ops
        return ops.knn_gather(x, idx, lengths)
    out = x[:, :, None, :].expand(N, M, K, U).gather(1, idx.long()[..., None].expand(N, L, K, U))
    if lengths is None:
        return out
    dead = torch.arange(K)[None, :] >= lengths.long()[:, None]                     # [N,K]
    return torch.where(dead[:, None, :, None], torch.zeros((), dtype=x.dtype), out)
