"""Mesh priors (csrc/acfm_mesh.hip) and the template fit (csrc/acfm_fit.hip)."""
import torch

from .. import _lib
from .base import _LOSS_CHAMFER, _LOSS_EDGE_LEN, _LOSS_NORMAL, _f32c, _row_scratch


# ------------------------------------------------------------------------------ mesh priors
def cot_laplacian(verts, faces):
    """Dense cot Laplacian L [V,V] of one mesh (verts [V,3], faces [F,3]); constant (no grad)."""
    _lib.require_gpu(verts, faces)
    v = _f32c(verts)
    f = faces.detach().to(torch.int64).contiguous()
    V, F = v.shape[0], f.shape[0]
    L = torch.empty((V, V), dtype=torch.float32, device=v.device)
    _lib.call("acfm_cot_laplacian", v.device, v, f, V, F, L)
    return L


class _LaplacianSmoothing(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts_packed, conn, vweight, method, vpm=0, fpm=0):
        _lib.require_gpu(verts_packed, conn, vweight)
        v, w = _f32c(verts_packed), _f32c(vweight)
        c = conn.detach().to(torch.int64).contiguous()
        P, F = v.shape[0], c.shape[0]
        n = _lib.lib().acfm_laplacian_smoothing_state_floats(P, F)
        state = torch.empty(n, dtype=torch.float32, device=v.device)
        loss = torch.empty((), dtype=torch.float32, device=v.device)
        _lib.call("acfm_laplacian_smoothing", v.device, v, c, w, P, F, int(method), int(vpm), int(fpm), loss, state)
        ctx.save_for_backward(c, state)
        ctx.cfg = (P, F, int(method), int(vpm), int(fpm))
        return loss

    @staticmethod
    def backward(ctx, go):
        c, state = ctx.saved_tensors
        P, F, method, vpm, fpm = ctx.cfg
        g = _f32c(go).reshape(1)
        gv = torch.empty((P, 3), dtype=torch.float32, device=g.device)
        _lib.call("acfm_laplacian_smoothing_backward", g.device, c, state, g, P, F, method, vpm, fpm, gv)
        return gv, None, None, None, None, None


def laplacian_smoothing_sum(verts_packed, conn, vweight, method, verts_per_mesh=0, faces_per_mesh=0):
    """sum_v vweight[v] * |L v|_v on packed meshes; method 0 = cot (conn = faces), 1 = uniform
    (conn = unique edges).  verts_per_mesh / faces_per_mesh: the packed arrays are equal-sized meshes
    one after the other (Meshes built from padded [N,V,3] / [N,F,3] tensors): per-mesh LDS kernels."""
    return _LaplacianSmoothing.apply(verts_packed, conn, vweight, method, verts_per_mesh, faces_per_mesh)


class _EdgeRigidity(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts, edges, verts_t, edges_t, vpm=0):
        _lib.require_gpu(verts, edges, verts_t, edges_t)
        v, vt = _f32c(verts), _f32c(verts_t)
        e = edges.detach().to(torch.int64).contiguous()
        et = edges_t.detach().to(torch.int64).contiguous()
        if e.shape != et.shape:
            raise ValueError("meshes and template must have the same number of edges")
        loss = torch.empty((), dtype=torch.float32, device=v.device)
        _lib.call("acfm_edge_rigidity", v.device, v, e, vt, et, e.shape[0], loss)
        ctx.save_for_backward(v, e, vt, et)
        ctx.vpm = int(vpm)
        return loss

    @staticmethod
    def backward(ctx, go):
        v, e, vt, et = ctx.saved_tensors
        g = _f32c(go).reshape(1)
        gv = torch.empty_like(v) if ctx.needs_input_grad[0] else None
        gvt = torch.empty_like(vt) if ctx.needs_input_grad[2] else None
        _lib.call("acfm_edge_rigidity_backward", g.device, v, e, vt, et, e.shape[0], v.shape[0], vt.shape[0], ctx.vpm,
                  g, gv, gvt)
        return gv, None, gvt, None, None


def edge_rigidity_sum(verts_packed, edges, verts_t_packed, edges_t, verts_per_mesh=0):
    """sum_e (|v[e0]-v[e1]| - |vt[et0]-vt[et1]|)^2 on packed meshes.  verts_per_mesh > 0: equal-sized
    meshes and `edges` sorted by its first vertex (Meshes.edges_packed()): the backward accumulates per
    mesh in LDS instead of with global atomics."""
    return _EdgeRigidity.apply(verts_packed, edges, verts_t_packed, edges_t, verts_per_mesh)


# ------------------------------------------------------------------------------ template fit (csrc/acfm_fit.hip)
def _lengths(lengths, N, P, device, what):
    if lengths is None:
        return None
    if lengths.shape != (N,):
        raise ValueError("%s must have shape (N,) = (%d,), got %s" % (what, N, tuple(lengths.shape)))
    _lib.require_gpu(lengths)
    return lengths.detach().to(torch.int64).contiguous()


class _Chamfer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, x_lengths, y_lengths):
        _lib.require_gpu(x, y)
        a, b = _f32c(x), _f32c(y)
        N, P1, _ = a.shape
        P2 = b.shape[1]
        xl, yl = _lengths(x_lengths, N, P1, a.device, "x_lengths"), _lengths(y_lengths, N, P2, a.device, "y_lengths")
        sums = torch.empty((N, 2), dtype=torch.float32, device=a.device)
        ix = torch.empty((N, P1), dtype=torch.int32, device=a.device)
        iy = torch.empty((N, P2), dtype=torch.int32, device=a.device)
        with torch.cuda.device(a.device):
            need = int(_lib.lib().acfm_chamfer_partial_floats(N, P1, P2))
            tk, part, nf = _row_scratch(a.device, _LOSS_CHAMFER, 2 * N, need)
        _lib.call("acfm_chamfer", a.device, a, b, xl, yl, N, P1, P2, sums, ix, iy, tk, part, nf)
        ctx.save_for_backward(a, b, ix, iy)
        ctx.lens = (xl, yl)
        ctx.mark_non_differentiable(ix, iy)
        return sums, ix, iy

    @staticmethod
    def backward(ctx, gs, _gix, _giy):
        a, b, ix, iy = ctx.saved_tensors
        xl, yl = ctx.lens
        N, P1, _ = a.shape
        P2 = b.shape[1]
        g = _f32c(gs)
        ga, gb = torch.empty_like(a), torch.empty_like(b)
        _lib.call("acfm_chamfer_backward", a.device, a, b, xl, yl, ix, iy, g, N, P1, P2, ga, gb)
        return ga, gb, None, None


def chamfer_nearest(x, y, x_lengths=None, y_lengths=None):
    """x [N,P1,3], y [N,P2,3] (+ int lengths [N] on the device, or None) -> (sums [N,2], idx_x [N,P1] i32, idx_y [N,P2]
    i32): sums[n,0] = sum_{i < x_len} min_{j < y_len} |x_i - y_j|^2, sums[n,1] its mirror image; the indices of the
    nearest points (lowest index among equal distances; rows at or past a length hold no value).  The sums are
    bit-reproducible, their gradients are not (float atomics in the backward)."""
    if x.dim() != 3 or y.dim() != 3 or x.shape[2] != 3 or y.shape[2] != 3 or x.shape[0] != y.shape[0]:
        raise ValueError("chamfer: x [N,P1,3] and y [N,P2,3] expected, got %s and %s" % (tuple(x.shape), tuple(y.shape)))
    if x.shape[0] == 0 or x.shape[1] == 0 or y.shape[1] == 0:
        raise ValueError("chamfer: x and y must hold at least one cloud of at least one point each")
    return _Chamfer.apply(x, y, x_lengths, y_lengths)


def chamfer_sums(x, y, x_lengths=None, y_lengths=None):
    return chamfer_nearest(x, y, x_lengths, y_lengths)[0]


class _EdgeLength(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts, edges, eweight, target):
        _lib.require_gpu(verts, edges, eweight)
        v, w = _f32c(verts), _f32c(eweight)
        e = edges.detach().to(torch.int64).contiguous()
        P, E = v.shape[0], e.shape[0]
        loss = torch.empty((), dtype=torch.float32, device=v.device)
        with torch.cuda.device(v.device):
            tk, part, nf = _row_scratch(v.device, _LOSS_EDGE_LEN, 1, int(_lib.lib().acfm_mesh_term_partial_floats(E)))
        _lib.call("acfm_edge_length_loss", v.device, v, e, w, P, E, float(target), loss, tk, part, nf)
        ctx.save_for_backward(v, e, w)
        ctx.target = float(target)
        return loss

    @staticmethod
    def backward(ctx, go):
        v, e, w = ctx.saved_tensors
        g = _f32c(go).reshape(1)
        gv = torch.empty_like(v)
        _lib.call("acfm_edge_length_loss_backward", v.device, v, e, w, g, v.shape[0], e.shape[0], ctx.target, gv)
        return gv, None, None, None


def edge_length_sum(verts_packed, edges, eweight, target_length=0.0):
    """sum_e eweight[e] (|v[e0] - v[e1]| - target_length)^2 on packed meshes (verts [P,3], edges [E,2], E > 0)."""
    return _EdgeLength.apply(verts_packed, edges, eweight, target_length)


class _NormalConsistency(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts, quads, qweight):
        _lib.require_gpu(verts, quads, qweight)
        v, w = _f32c(verts), _f32c(qweight)
        q = quads.detach().to(torch.int64).contiguous()
        P, Q = v.shape[0], q.shape[0]
        loss = torch.empty((), dtype=torch.float32, device=v.device)
        with torch.cuda.device(v.device):
            tk, part, nf = _row_scratch(v.device, _LOSS_NORMAL, 1, int(_lib.lib().acfm_mesh_term_partial_floats(Q)))
        _lib.call("acfm_normal_consistency", v.device, v, q, w, P, Q, loss, tk, part, nf)
        ctx.save_for_backward(v, q, w)
        return loss

    @staticmethod
    def backward(ctx, go):
        v, q, w = ctx.saved_tensors
        g = _f32c(go).reshape(1)
        gv = torch.empty_like(v)
        _lib.call("acfm_normal_consistency_backward", v.device, v, q, w, g, v.shape[0], q.shape[0], gv)
        return gv, None, None


def normal_consistency_sum(verts_packed, quads, qweight):
    """sum_q qweight[q] (1 - cos(n0, n1)) over the pairs of faces (a, b, c), (a, b, d) on an edge: quads [Q,4] =
    (a, b, c, d), Q > 0 (Meshes.normal_pairs_packed() builds them)."""
    return _NormalConsistency.apply(verts_packed, quads, qweight)
