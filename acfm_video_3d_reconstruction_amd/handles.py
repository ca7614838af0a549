"""The handle weights `lbs` of MeshNet as the reference initialises them (multiframe/nnutils/mesh_net.py:54-85,
523-544): farthest-point sampling over the GEODESIC distance matrix of the template, then log(clamp(1 / d ** 16)).

The reference takes the distances from gdist.local_gdist_matrix (exact polyhedral geodesics).  Here they are shortest
paths on the edge-Steiner graph of the mesh (DESIGN.md "Geodesic handles"): `steiner` = m points on every edge, inside
every face all pairs of its 3 + 3 m boundary nodes joined by their Euclidean distance.  That is an upper bound of the
exact geodesic that converges to it with m (under 0.2 % at the default m = 15), NOT gdist's values; nothing here could
be checked against the gdist package.

GPU tensors run ops.geodesic_distances (csrc/acfm_geodesic.hip, float32).  Arrays and host tensors take the same graph
through scipy.sparse.csgraph.dijkstra in float64 -- for building and checking without a GPU, as the host branch of
flow_ops is."""
import numpy as np
import torch

MAX_STEINER = 20     # 3 m + 3 boundary nodes of a face fit one wave of the kernel; the host path keeps the same bound


def _steiner(steiner):
    m = int(steiner)
    if m != steiner or not 0 <= m <= MAX_STEINER:
        raise ValueError("steiner must be an integer in [0, %d], got %r" % (MAX_STEINER, steiner))
    return m


def edge_tables(faces, V):
    """faces [F,3] integer array -> (edges [E,2] = (lo, hi) in Meshes.edges_packed() order, face_edges [F,3] = the rows
    of `edges` of each face's edges v1v2, v2v0, v0v1), int64."""
    f = np.asarray(faces)
    if f.ndim != 2 or f.shape[1] != 3 or f.shape[0] < 1 or not np.issubdtype(f.dtype, np.integer):
        raise ValueError("faces: [F,3] of integers expected, got %s %s" % (f.dtype, f.shape))
    f = f.astype(np.int64)
    if f.min() < 0 or f.max() >= V:
        raise ValueError("faces hold vertex ids in [%d, %d], the mesh has %d vertices" % (f.min(), f.max(), V))
    a, b = f[:, [1, 2, 0]], f[:, [2, 0, 1]]
    key = np.minimum(a, b) * V + np.maximum(a, b)
    uniq = np.unique(key)
    return np.stack([uniq // V, uniq % V], 1), np.searchsorted(uniq, key)


def steiner_graph(verts, faces, steiner):
    """The edge-Steiner graph as (positions [V + m E, 3] float64, rows, cols, lengths): every undirected arc once, rows
    < cols.  Node V + e m + (j - 1), j = 1..m, sits at a + (j / (m + 1)) (b - a) on edge e = (a, b)."""
    m = _steiner(steiner)
    v = np.asarray(verts, np.float64)
    if v.ndim != 2 or v.shape[1] != 3 or v.shape[0] < 1:
        raise ValueError("verts: [V,3] expected, got %s" % (v.shape,))
    if not np.isfinite(v).all():
        raise ValueError("verts hold positions that are not finite")
    V = v.shape[0]
    edges, face_edges = edge_tables(faces, V)
    f = np.asarray(faces).astype(np.int64)
    E = edges.shape[0]
    t = (np.arange(1, m + 1, dtype=np.float64) / (m + 1))[None, :, None]
    a, b = v[edges[:, 0]][:, None], v[edges[:, 1]][:, None]
    pos = np.concatenate([v, (a + t * (b - a)).reshape(E * m, 3)], 0)
    # the boundary nodes of every face, in the kernel's lane order: its vertices, then the m points of each edge
    on_edges = V + face_edges[:, :, None] * m + np.arange(m)[None, None]
    ids = np.concatenate([f, on_edges.reshape(f.shape[0], 3 * m)], 1)
    p, q = np.triu_indices(ids.shape[1], 1)
    r, c = ids[:, p].reshape(-1), ids[:, q].reshape(-1)
    r, c = np.minimum(r, c), np.maximum(r, c)
    # an arc on an edge shared by two faces comes twice (a sparse matrix would ADD the two), a degenerate face has loops
    key = np.unique((r * pos.shape[0] + c)[r != c])
    r, c = key // pos.shape[0], key % pos.shape[0]
    return pos, r, c, np.linalg.norm(pos[r] - pos[c], axis=1)


def _host_distances(verts, faces, m, sources):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra
    pos, r, c, w = steiner_graph(verts, faces, m)
    V, n = np.asarray(verts).shape[0], pos.shape[0]
    if sources is None:
        src = np.arange(V)
    else:
        src = np.asarray(sources).astype(np.int64).reshape(-1)
        if src.size < 1 or src.min() < 0 or src.max() >= V:
            raise ValueError("sources: at least one vertex id in [0, %d) expected" % V)
    # (explicit zeros stay in the matrix: two nodes at one position are joined by an arc of length 0)
    g = csr_matrix((w, (r, c)), shape=(n, n))
    return dijkstra(g, directed=False, indices=src)[:, :V]


MEMORY = ("lds", "device", "auto")   # ops.GEODESIC_MEMORY (this module imports without the library)


def _memory(memory):
    if memory not in MEMORY:
        raise ValueError('memory must be one of "lds", "device", "auto", got %r' % (memory,))
    return memory


def geodesic_distance_matrix(verts, faces, steiner=15, sources=None, memory="auto"):
    """D [S,V]: D[s,v] = the edge-Steiner distance from vertex sources[s] (None = all V) to vertex v, +inf between
    components.  GPU tensors -> ops.geodesic_distances (float32 tensor on the device; verts may be [N,V,3]); arrays or
    host tensors -> float64 through scipy (an array for arrays, a tensor for tensors).
    memory: where the GPU kernel keeps the node distances -- "lds" (refused when the graph does not fit a workgroup's
    LDS), "device" (a workspace, any graph) or "auto" (LDS where it fits: the same bits either way).  The host path
    only validates it."""
    m = _steiner(steiner)
    _memory(memory)
    if torch.is_tensor(verts) and verts.is_cuda:
        from . import ops
        f = faces if torch.is_tensor(faces) else torch.as_tensor(np.asarray(faces), device=verts.device)
        return ops.geodesic_distances(verts, f, m, sources, memory=memory)
    as_tensor = torch.is_tensor(verts)
    v = verts.detach().cpu().numpy() if torch.is_tensor(verts) else verts
    f = faces.detach().cpu().numpy() if torch.is_tensor(faces) else faces
    s = sources.detach().cpu().numpy() if torch.is_tensor(sources) else sources
    D = _host_distances(v, f, m, s)
    return torch.from_numpy(D) if as_tensor else D


def farthest_point_sampling(D, num_samples, start=0):
    """mesh_net.py:54-85 on a distance matrix D [V,V]: far = D[start]; then num_samples times far = min(far, D[s]),
    s = argmax(far) (the first maximum).  -> the num_samples + 1 indices, beginning with `start`, int64."""
    D = D.detach().cpu().numpy() if torch.is_tensor(D) else np.asarray(D)
    if D.ndim != 2 or D.shape[0] != D.shape[1] or D.shape[0] < 1:
        raise ValueError("D: a square distance matrix expected, got %s" % (D.shape,))
    s = int(start)
    if not 0 <= s < D.shape[0]:
        raise ValueError("start must lie in [0, %d), got %d" % (D.shape[0], s))
    far = D[s].copy()
    selected = [s]
    for _ in range(int(num_samples)):
        far = np.minimum(far, D[s])
        s = int(np.argmax(far))
        selected.append(s)
    return np.asarray(selected, np.int64)


def lbs_logits_from_distances(D, idx_pts, pp=16):
    """mesh_net.py:529-542 on D [V,V] (array or tensor) and the sorted handle vertices: w = 1 / d ** pp in float32 with
    d = D[:, idx_pts], infinities set to 0, w[idx_pts[i], i] = max(w[:, i]), log(clamp(w, 1e-10)) -> tensor [V,K] float32
    on D's device."""
    D = D if torch.is_tensor(D) else torch.from_numpy(np.asarray(D))
    idx = torch.as_tensor(np.asarray(idx_pts), dtype=torch.int64, device=D.device)
    d = D[:, idx].float()
    if bool(torch.isinf(d).any()):
        raise ValueError("the mesh is not connected: %d vertices cannot be reached from every handle"
                         % int(torch.isinf(d).any(1).sum()))
    w = 1 / d ** pp
    w[torch.isinf(w)] = 0
    w[idx, torch.arange(idx.numel(), device=D.device)] = w.max(dim=0)[0]
    return torch.log(torch.clamp(w, min=1e-10))


def geodesic_lbs_logits(verts, faces, num_lbs, pp=16, steiner=15, memory="auto"):
    """mesh_net.py:523-544: idx_pts = sorted(farthest_point_sampling(D, num_lbs - 1)), D the distance matrix of the
    template; logits = log(clamp(1 / D[:, idx_pts] ** pp, 1e-10)) with each handle's own row at its column maximum.
    -> (logits [V,num_lbs] float32 -- a tensor on verts' device for tensors, an array for arrays --, idx_pts int64 array).
    The logits are what deform.DeformSolver / MultiframeStep take as lbs_logits.  ValueError on a mesh that is not
    connected.  memory: as geodesic_distance_matrix (with "auto" the 2562-vertex template runs at the default steiner)."""
    _memory(memory)
    num_lbs = int(num_lbs)
    if num_lbs < 1:
        raise ValueError("num_lbs must be at least 1, got %d" % num_lbs)
    if (verts.dim() if torch.is_tensor(verts) else np.asarray(verts).ndim) != 2:
        raise ValueError("geodesic_lbs_logits: one template, verts [V,3], expected")
    D = geodesic_distance_matrix(verts, faces, steiner, memory=memory)
    idx_pts = np.sort(farthest_point_sampling(D, num_lbs - 1))
    logits = lbs_logits_from_distances(D, idx_pts, pp)
    return (logits if torch.is_tensor(verts) else logits.numpy()), idx_pts
