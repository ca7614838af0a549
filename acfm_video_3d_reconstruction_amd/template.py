"""The symmetric template of the reference's default configuration (--symmetric True, mesh_net.py:462-484, 573-595).

create_sphere / make_symmetric build the mean shape's mesh with its vertices ordered [independent (x == 0) |
right (x > 0) | left] and its faces ordered [independent | right | left]; the learned parameter holds the first
num_indept + num_sym rows only and symmetrize() appends the left half as (-x, y, z) of the right half, so the mean
shape is mirror-symmetric by construction.  A checkpoint stores that half parameter but no faces: the faces are
rebuilt by these two functions, whose vertex and face ORDER is therefore part of the checkpoint format
(tests/golden/symmetric_template.npz pins it against the reference's own output).

Host code, numpy; symmetrize() alone takes tensors and sends GPU tensors to ops.symmetrize (csrc/acfm_deform.hip)."""
import numpy as np
import torch

_T = (1.0 + np.sqrt(5.0)) / 2.0
# the icosahedron the subdivision starts from (utils/meshzoo.py: the order of these two tables fixes every later index)
_ICO_VERTS = ((-1, _T, 0), (1, _T, 0), (-1, -_T, 0), (1, -_T, 0), (0, -1, _T), (0, 1, _T), (0, -1, -_T), (0, 1, -_T),
              (_T, 0, -1), (_T, 0, 1), (-_T, 0, -1), (-_T, 0, 1))
_ICO_FACES = ((0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
              (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10),
              (8, 6, 7), (9, 8, 1))


def _subdivide(verts, tris, tri_edges):
    """One 1 -> 4 split.  tri_edges[t] lists triangle t's three edges (vertex pairs) in the order in which they are
    visited: a midpoint gets the next free index the first time its edge is visited, triangles in order, edges in
    that order.  The order is what the reference's numbering follows, and it is NOT "edge k opposite corner k" after
    the first split (see the corner triangles below), so it is carried along explicitly."""
    verts = list(verts)
    mid_of = {}
    new_tris, new_edges = [], []
    for tri, edges in zip(tris, tri_edges):
        mids = []
        for a, b in edges:
            key = (a, b) if a < b else (b, a)
            if key not in mid_of:
                mid_of[key] = len(verts)
                verts.append(0.5 * (verts[a] + verts[b]))
            mids.append(mid_of[key])
        # for every corner, the midpoints of the two edges that meet there, in visiting order
        near = [[m for m, e in zip(mids, edges) if c in e] for c in tri]
        new_tris.append(tuple(mids))
        new_edges.append(tuple(tuple(near[k]) for k in range(3)))
        for k, c in enumerate(tri):
            p, q = near[k]
            new_tris.append((c, p, q))
            new_edges.append(((p, q), (c, p), (c, q)))
    return verts, new_tris, new_edges


def create_sphere(n_subdivide=3):
    """The unit icosphere with the reference's vertex and face order (utils/mesh.py:12-16 over utils/meshzoo.py's
    iso_sphere): -> verts [V,3] float64, faces [F,3] int64; 42/80, 162/320, 642/1280, 2562/5120 at levels 1..4.
    Midpoints are formed on the flat faces of every level and all vertices are pushed to the sphere once, at the end."""
    verts = [np.array(v, dtype=np.float64) for v in _ICO_VERTS]
    tris = list(_ICO_FACES)
    edges = [((t[1], t[2]), (t[2], t[0]), (t[0], t[1])) for t in tris]    # edge k lies opposite corner k
    for _ in range(int(n_subdivide)):
        verts, tris, edges = _subdivide(verts, tris, edges)
    v = np.stack(verts)
    v = v / np.sqrt(np.einsum("ij,ij->i", v, v))[:, None]
    return v, np.array(tris, dtype=np.int64)


def make_symmetric(verts, faces):
    """Reorder a mesh that is exactly mirror-symmetric in x (utils/mesh.py:19-154):
    -> (verts, faces, num_indept, num_sym, num_indept_faces, num_sym_faces) with
    verts = [x == 0 | x > 0 | their mirror images, in the same order], each group in its original order, and
    faces = [independent (their own mirror image) | right | left], where left face i lists the mirror images of
    right face i's vertices in the same order.
    Raises ValueError naming the first vertex that has no exact mirror image."""
    verts = np.asarray(verts)
    faces = np.asarray(faces)
    x = verts[:, 0]
    centre, right = np.nonzero(x == 0)[0], np.nonzero(x > 0)[0]
    where = {tuple(p): i for i, p in enumerate(verts.tolist())}
    image = [where.get((-p[0], p[1], p[2])) for p in verts.tolist()]
    for i, j in enumerate(image):
        if j is None:      # (the reference stops in a debugger here)
            raise ValueError("make_symmetric: the mesh is not mirror-symmetric in x: vertex %d at %r has no mirror "
                             "image (-x, y, z)" % (i, tuple(verts[i].tolist())))
    left = [image[i] for i in right]
    n_indept, n_sym = len(centre), len(right)
    order = np.concatenate([centre, right, np.array(left, dtype=np.int64)]).astype(np.int64)
    rank = np.empty(len(verts), dtype=np.int64)
    rank[order] = np.arange(len(verts))
    verts, faces = verts[order], rank[faces]

    mirror = np.arange(len(verts))
    mirror[n_indept:n_indept + n_sym] += n_sym
    mirror[n_indept + n_sym:] -= n_sym
    at = {tuple(sorted(f)): i for i, f in enumerate(faces.tolist())}
    done = np.zeros(len(faces), dtype=bool)
    f_indept, f_right, f_left = [], [], []
    for i, face in enumerate(faces):
        if done[i]:
            continue
        twin = mirror[face]
        ids, twin_ids = np.sort(face), np.sort(twin)
        done[i] = True
        if (ids == twin_ids).all():
            f_indept.append(face)
            continue
        done[at[tuple(twin_ids.tolist())]] = True
        # Which of the pair is the left one is read off the x coordinates at the positions where the SORTED index
        # lists differ, applied to the face's own (unsorted) order -- the reference's test as it stands; it decides
        # the order of the fixture, so it is kept to the letter
        differ = ids != twin_ids
        if (verts[face][differ, 0] < verts[twin][differ, 0]).all():
            f_left.append(face); f_right.append(twin)
        else:
            f_left.append(twin); f_right.append(face)
    out = np.array(f_indept + f_right + f_left, dtype=np.int64).reshape(-1, 3)
    return verts, out, n_indept, n_sym, len(f_indept), len(f_right)


def fold(grad_full, num_sym):
    """The gradient of symmetrize(): [.., n_half + num_sym, 3] -> [.., n_half, 3], the left rows' gradient added to
    the right rows' with x negated.  (GPU tensors: one launch, acfm_symmetrize_backward.)"""
    if num_sym == 0:
        return grad_full
    if grad_full.is_cuda:
        from . import ops
        return ops.symmetrize_fold(grad_full, num_sym)
    n_half = grad_full.shape[-2] - num_sym
    flip = torch.ones((1, 3), dtype=grad_full.dtype)
    flip[0, 0] = -1
    out = grad_full[..., :n_half, :].clone()
    out[..., n_half - num_sym:, :] += flip * grad_full[..., n_half:, :]
    return out


def symmetrize(V, num_sym):
    """MeshNet.symmetrize (mesh_net.py:573-591): V [n_half,3] or [B,n_half,3] -> [.., n_half + num_sym, 3], the last
    num_sym rows appended once more as (-x, y, z).  num_sym == 0 returns V itself.  GPU tensors go to ops.symmetrize
    (one launch each way), host tensors through the reference's torch lines."""
    if num_sym == 0:
        return V
    if V.is_cuda:
        from . import ops
        return ops.symmetrize(V, num_sym)
    flip = torch.ones((1, 3), device=V.device)
    flip[0, 0] = -1
    if V.dim() == 2:
        return torch.cat([V, flip * V[-num_sym:]], 0)
    return torch.cat([V, flip * V[:, -num_sym:]], 1)
