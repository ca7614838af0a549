"""pytorch3d.loss.mesh_laplacian_smoothing (called at multiframe/main.py:703 with 'cot',
monocular/main.py:276 with 'uniform'); semantics: SURVEY App-A.7.  chamfer_distance, mesh_edge_loss and
mesh_normal_consistency as utils/geometry.py:75-140 (fit_verts_to_mesh) calls them.  GPU tensors take the kernels of
csrc/acfm_fit.hip, host tensors the torch formulations below."""
import torch


def _cot_weights(verts, faces):
    """Per-face cotangents/4 exactly as geom_utils.laplacian_cot (geom_utils.py:272-298)."""
    fv = verts[faces]
    v0, v1, v2 = fv[:, 0], fv[:, 1], fv[:, 2]
    A = (v1 - v2).norm(dim=1)
    B = (v0 - v2).norm(dim=1)
    C = (v0 - v1).norm(dim=1)
    s = 0.5 * (A + B + C)
    area = (s * (s - A) * (s - B) * (s - C)).clamp_(min=1e-12).sqrt()
    A2, B2, C2 = A * A, B * B, C * C
    cot = torch.stack([(B2 + C2 - A2) / area, (A2 + C2 - B2) / area, (A2 + B2 - C2) / area], dim=1)
    return cot / 4.0


def mesh_laplacian_smoothing(meshes, method: str = "uniform"):
    if meshes.isempty():
        return torch.tensor([0.0], dtype=torch.float32, device=meshes.device, requires_grad=True)
    N = len(meshes)
    verts = meshes.verts_packed()
    faces = meshes.faces_packed()
    weights = meshes.inv_num_verts_packed()
    V = verts.shape[0]
    if verts.is_cuda and method in ("cot", "uniform"):
        from .. import ops  # fused gfx950 kernels (csrc/acfm_mesh.hip); torch ops below = host tensors
        conn = faces if method == "cot" else meshes.edges_packed()
        vpm = fpm = 0
        if method == "cot" and meshes._equal_sized():    # mesh m = verts [m V, (m+1) V), faces [m F, (m+1) F)
            vpm, fpm = meshes.verts_list()[0].shape[0], meshes.faces_list()[0].shape[0]
        return ops.laplacian_smoothing_sum(verts, conn, weights, 0 if method == "cot" else 1, vpm, fpm) / N
    if method == "uniform":
        L = meshes.laplacian_packed()
        loss = torch.sparse.mm(L, verts)
    elif method in ("cot", "cotcurv"):
        with torch.no_grad():
            cot = _cot_weights(verts.detach(), faces)                 # weights are constants
            ii = faces[:, [1, 2, 0]].reshape(-1)
            jj = faces[:, [2, 0, 1]].reshape(-1)
            w = cot.reshape(-1)
            rows = torch.cat([ii, jj])
            cols = torch.cat([jj, ii])
            ww = torch.cat([w, w])
            rowsum = torch.zeros(V, dtype=verts.dtype, device=verts.device).index_add_(0, rows, ww)
            if method == "cot":
                norm_w = torch.where(rowsum > 0, 1.0 / rowsum, rowsum).view(-1, 1)
            else:
                area = torch.zeros(V, dtype=verts.dtype, device=verts.device)
                fv = verts.detach()[faces]
                a = 0.5 * torch.cross(fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0], dim=1).norm(dim=1)
                area.index_add_(0, faces.reshape(-1), a.repeat_interleave(3))
                norm_w = 0.25 * torch.where(area > 0, 1.0 / area, area).view(-1, 1)
        Lv = torch.zeros_like(verts).index_add_(0, rows, ww[:, None] * verts[cols])   # (W v)
        loss = Lv * norm_w - verts if method == "cot" else (Lv - verts) * norm_w
    else:
        raise ValueError("Method should be one of {uniform, cot, cotcurv}")
    loss = loss.norm(dim=1) * weights
    return loss.sum() / N


def _zero(meshes):
    return torch.tensor([0.0], dtype=torch.float32, device=meshes.device, requires_grad=True)


def _chamfer_sums_host(x, y, xl, yl):
    """(sums [N,2], idx_x [N,P1], idx_y [N,P2]) as ops.chamfer_nearest, with torch ops: the nearest index is chosen
    under no_grad (first occurrence of the minimum; 0 where the other cloud is empty), the distance to it is
    differentiable."""
    N, P1, _ = x.shape
    P2 = y.shape[1]
    with torch.no_grad():
        dx = x[:, :, None, 0] - y[:, None, :, 0]
        dy = x[:, :, None, 1] - y[:, None, :, 1]
        dz = x[:, :, None, 2] - y[:, None, :, 2]
        d = (dx * dx + dy * dy) + dz * dz                                  # [N,P1,P2]
        vx = torch.arange(P1, device=x.device)[None] < xl[:, None]         # [N,P1] rows that count
        vy = torch.arange(P2, device=x.device)[None] < yl[:, None]
        inf = torch.full_like(d, float("inf"))
        d = torch.where(vx[:, :, None] & vy[:, None, :], d, inf)           # (padding may hold NaN: never compared)
        ix = torch.from_numpy(d.numpy().argmin(2))                         # numpy: the first minimum, as documented
        iy = torch.from_numpy(d.numpy().argmin(1))
        vx = vx & (yl > 0)[:, None]
        vy = vy & (xl > 0)[:, None]
    zero = torch.zeros((), dtype=x.dtype)
    ex = torch.where(vx[:, :, None], x, zero) - torch.where(vx[:, :, None], y.gather(1, ix[:, :, None].expand(-1, -1, 3)), zero)
    ey = torch.where(vy[:, :, None], y, zero) - torch.where(vy[:, :, None], x.gather(1, iy[:, :, None].expand(-1, -1, 3)), zero)
    cx = ((ex[..., 0] * ex[..., 0] + ex[..., 1] * ex[..., 1]) + ex[..., 2] * ex[..., 2]).sum(1)
    cy = ((ey[..., 0] * ey[..., 0] + ey[..., 1] * ey[..., 1]) + ey[..., 2] * ey[..., 2]).sum(1)
    return torch.stack([cx, cy], 1), ix, iy


def chamfer_distance(x, y, x_lengths=None, y_lengths=None, x_normals=None, y_normals=None, weights=None,
                     batch_reduction="mean", point_reduction="mean"):
    """-> (loss, loss_normals).  x [N,P1,3], y [N,P2,3] float32 tensors (Pointclouds are not supported); cham_x[n] =
    sum_{i < x_lengths[n]} min_{j < y_lengths[n]} |x_i - y_j|^2 and cham_y its mirror image, times weights[n]; divided by
    the lengths for point_reduction "mean"; summed over the batch for batch_reduction "sum", and divided by N (by
    weights.sum() with weights) for "mean"; loss = cham_x + cham_y.  A length of 0 gives a sum of 0 (and 0 / 0 under
    "mean").  Among equal distances the lowest index is the nearest neighbour.
    loss_normals is None unless x_normals [N,P1,3] and y_normals [N,P2,3] are both given; then it is formed as
    PyTorch3D forms it: per point 1 - |cosine_similarity(own normal, the nearest point's normal, eps=1e-6)| (knn_gather
    of the other cloud's normals by the nearest-neighbour indices; the normal of a point without a neighbour is 0, its
    term 1), rows at or past a length removed, then the weights and reductions of the distance term.  Gradients reach
    the normals; the points get none from this term (the index is an integer).  One of the two alone is refused."""
    if (x_normals is None) != (y_normals is None):
        raise ValueError("chamfer_distance: x_normals and y_normals must be given together (got only %s)"
                         % ("x_normals" if y_normals is None else "y_normals"))
    if batch_reduction is not None and batch_reduction not in ("mean", "sum"):
        raise ValueError('batch_reduction must be one of ["mean", "sum"] or None')
    if point_reduction not in ("mean", "sum"):
        raise ValueError('point_reduction must be one of ["mean", "sum"]')
    if not torch.is_tensor(x) or not torch.is_tensor(y):
        raise ValueError("chamfer_distance: x and y must be tensors (Pointclouds are not supported)")
    if x.dim() != 3 or x.shape[2] != 3:
        raise ValueError("chamfer_distance: x must have shape (N, P1, 3), got %s" % (tuple(x.shape),))
    if y.dim() != 3 or y.shape[2] != 3 or y.shape[0] != x.shape[0]:
        raise ValueError("chamfer_distance: y must have shape (N, P2, 3) with x's N, got %s" % (tuple(y.shape),))
    N, P1, P2 = x.shape[0], x.shape[1], y.shape[1]
    for name, t in (("x_lengths", x_lengths), ("y_lengths", y_lengths), ("weights", weights)):
        if t is not None and tuple(t.shape) != (N,):
            raise ValueError("chamfer_distance: %s must have shape (N,) = (%d,)" % (name, N))
    if x_normals is not None:
        if tuple(x_normals.shape) != tuple(x.shape) or tuple(y_normals.shape) != tuple(y.shape):
            raise ValueError("chamfer_distance: x_normals / y_normals must have the shapes of x / y, got %s and %s"
                             % (tuple(x_normals.shape), tuple(y_normals.shape)))
    if x.is_cuda:
        from .. import ops
        sums, ix, iy = ops.chamfer_nearest(x, y, x_lengths, y_lengths)
    else:
        xl = torch.full((N,), P1, dtype=torch.int64) if x_lengths is None else x_lengths.long().clamp(0, P1)
        yl = torch.full((N,), P2, dtype=torch.int64) if y_lengths is None else y_lengths.long().clamp(0, P2)
        sums, ix, iy = _chamfer_sums_host(x.float(), y.float(), xl, yl)

    def reduce(cham_x, cham_y):
        if weights is not None:
            cham_x, cham_y = cham_x * weights, cham_y * weights
        if point_reduction == "mean":
            cham_x = cham_x / (float(P1) if x_lengths is None else x_lengths.to(cham_x.dtype))
            cham_y = cham_y / (float(P2) if y_lengths is None else y_lengths.to(cham_y.dtype))
        if batch_reduction is not None:
            cham_x, cham_y = cham_x.sum(), cham_y.sum()
            if batch_reduction == "mean":
                div = weights.sum() if weights is not None else float(N)
                cham_x, cham_y = cham_x / div, cham_y / div
        return cham_x + cham_y

    loss = reduce(sums[:, 0], sums[:, 1])
    if x_normals is None:
        return loss, None
    return loss, reduce(_normal_sums(x_normals, y_normals, ix, x_lengths, y_lengths),
                        _normal_sums(y_normals, x_normals, iy, y_lengths, x_lengths))


def _normal_sums(own, other, idx, own_lengths, other_lengths):
    """[N]: sum over the rows inside own_lengths of 1 - |cos(own normal, other[idx])|.  idx [N,P] are the nearest
    neighbours' indices; rows at or past a length (which may hold NaN, and an unwritten index) leave through `where`."""
    from .ops import knn_gather
    near = knn_gather(other, idx[:, :, None], other_lengths)[:, :, 0]
    if own_lengths is None:
        return (1.0 - torch.nn.functional.cosine_similarity(own, near, dim=2, eps=1e-6).abs()).sum(1)
    # the padded rows leave before the cosine as well: behind it a NaN would come back as 0 x NaN in the backward
    live = torch.arange(own.shape[1], device=own.device)[None] < own_lengths[:, None]
    zero = torch.zeros((), dtype=own.dtype, device=own.device)
    own, near = torch.where(live[:, :, None], own, zero), torch.where(live[:, :, None], near, zero)
    term = 1.0 - torch.nn.functional.cosine_similarity(own, near, dim=2, eps=1e-6).abs()
    return torch.where(live, term, zero).sum(1)


def mesh_edge_loss(meshes, target_length: float = 0.0):
    """sum_e w_e (|v_a - v_b| - target_length)^2 / N over edges_packed(), w_e = 1 / (edges of the edge's mesh)."""
    if meshes.isempty():
        return _zero(meshes)
    N = len(meshes)
    verts, edges = meshes.verts_packed(), meshes.edges_packed()
    if edges.shape[0] == 0:
        return _zero(meshes)
    w = meshes.inv_num_edges_packed()
    if verts.is_cuda:
        from .. import ops
        return ops.edge_length_sum(verts, edges, w, target_length) / N
    d = verts[edges[:, 0]] - verts[edges[:, 1]]
    return (((d.norm(dim=1) - target_length) ** 2.0) * w).sum() / N


def mesh_normal_consistency(meshes):
    """sum over the pairs of faces that share an edge of (1 - cos(n0, n1)) / (pairs of the mesh), / N; an edge in m
    faces gives m (m - 1) / 2 pairs (Meshes.normal_pairs_packed())."""
    if meshes.isempty():
        return _zero(meshes)
    N = len(meshes)
    verts = meshes.verts_packed()
    quads, w = meshes.normal_pairs_packed()
    if quads.shape[0] == 0:
        return _zero(meshes)
    if verts.is_cuda:
        from .. import ops
        return ops.normal_consistency_sum(verts, quads, w) / N
    a = verts[quads[:, 0]]
    eb, ec, ed = verts[quads[:, 1]] - a, verts[quads[:, 2]] - a, verts[quads[:, 3]] - a
    n0, n1 = torch.cross(ec, eb, dim=1), -torch.cross(ed, eb, dim=1)
    cos = (n0 * n1).sum(1) / (n0.norm(dim=1) * n1.norm(dim=1)).clamp(min=1e-8)
    return ((1.0 - cos) * w).sum() / N
