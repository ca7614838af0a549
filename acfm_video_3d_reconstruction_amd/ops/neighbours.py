"""K nearest neighbours and gather by neighbour index (csrc/acfm_knn.hip): PyTorch3D 0.3.0's pytorch3d.ops.knn."""
import torch

from .. import _lib
from .mesh_terms import _lengths

KNN_MAX_K = 32


class _KnnPoints(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p1, p2, lengths1, lengths2, K):
        a, b = p1.detach().contiguous(), p2.detach().contiguous()
        N, P1, _ = a.shape
        P2 = b.shape[1]
        l1, l2 = _lengths(lengths1, N, P1, a.device, "lengths1"), _lengths(lengths2, N, P2, a.device, "lengths2")
        dists = torch.empty((N, P1, K), dtype=torch.float32, device=a.device)
        idx = torch.empty((N, P1, K), dtype=torch.int64, device=a.device)
        _lib.call("acfm_knn_points", a.device, a, b, l1, l2, N, P1, P2, K, dists, idx)
        ctx.save_for_backward(a, b, idx)
        ctx.lens = (l1, l2)
        ctx.mark_non_differentiable(idx)
        ctx.set_materialize_grads(False)      # (or the engine forms an [N,P1,K] int64 zero "gradient" for idx)
        return dists, idx

    @staticmethod
    def backward(ctx, gd, _gi):
        if gd is None:
            return None, None, None, None, None
        a, b, idx = ctx.saved_tensors
        l1, l2 = ctx.lens
        N, P1, K = idx.shape
        g = gd.detach().to(torch.float32).contiguous()
        ga, gb = torch.empty_like(a), torch.empty_like(b)
        _lib.call("acfm_knn_points_backward", a.device, a, b, l1, l2, idx, g, N, P1, b.shape[1], K, ga, gb)
        return ga, gb, None, None, None


def knn_points(p1, p2, lengths1=None, lengths2=None, K=1):
    """p1 [N,P1,3], p2 [N,P2,3] float32 on the GPU (+ int lengths [N] on the device, or None), 1 <= K <= 32 ->
    (dists [N,P1,K] float32, idx [N,P1,K] int64): for every point of p1 inside lengths1 its min(K, lengths2[n]) nearest
    points of p2[n, :lengths2[n]] -- squared distances (dx dx + dy dy) + dz dz, ascending, the lower index first among
    equal distances -- and their indices.  Every other slot (rows at or past lengths1, columns at or past lengths2) holds
    0 / 0; rows at or past a length are never read.  The forward is bit-reproducible.  dists is differentiable in p1
    and p2; the gradient of p2 is summed with float atomics and is not bit-reproducible.  idx is not differentiable."""
    _lib.require_gpu(p1, p2)
    if p1.dim() != 3 or p2.dim() != 3 or p1.shape[2] != 3 or p2.shape[2] != 3 or p1.shape[0] != p2.shape[0]:
        raise ValueError("knn_points: p1 [N,P1,3] and p2 [N,P2,3] expected on the GPU (the kernels are written for "
                         "D = 3), got %s and %s" % (tuple(p1.shape), tuple(p2.shape)))
    if p1.dtype != torch.float32 or p2.dtype != torch.float32:
        raise ValueError("knn_points: p1 and p2 must be float32, got %s and %s" % (p1.dtype, p2.dtype))
    if int(K) != K or not 1 <= K <= KNN_MAX_K:
        raise ValueError("knn_points: K must be in 1..%d, got %r" % (KNN_MAX_K, K))
    if p1.shape[0] == 0 or p1.shape[1] == 0 or p2.shape[1] == 0:
        raise ValueError("knn_points: p1 and p2 must hold at least one cloud of at least one point each (N, P1, P2 > 0)")
    return _KnnPoints.apply(p1, p2, lengths1, lengths2, int(K))


class _KnnGather(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, idx, lengths):
        a, i = x.detach().contiguous(), idx.detach().contiguous()
        N, M, U = a.shape
        _, L, K = i.shape
        ln = _lengths(lengths, N, M, a.device, "lengths")
        out = torch.empty((N, L, K, U), dtype=torch.float32, device=a.device)
        _lib.call("acfm_knn_gather", a.device, a, i, int(i.dtype == torch.int64), ln, N, M, U, L, K, out)
        ctx.save_for_backward(i)
        ctx.cfg = (ln, N, M, U, L, K)
        return out

    @staticmethod
    def backward(ctx, go):
        (i,) = ctx.saved_tensors
        ln, N, M, U, L, K = ctx.cfg
        g = go.detach().to(torch.float32).contiguous()
        gx = torch.empty((N, M, U), dtype=torch.float32, device=g.device)
        _lib.call("acfm_knn_gather_backward", g.device, g, i, int(i.dtype == torch.int64), ln, N, M, U, L, K, gx)
        return gx, None, None


def knn_gather(x, idx, lengths=None):
    """x [N,M,U] float32, idx [N,L,K] int64 or int32, lengths [N] of x's clouds or None, all on the GPU ->
    [N,L,K,U] with out[n,l,k] = x[n, idx[n,l,k]].  Zeros where k >= lengths[n] or the index is outside [0, M): such an
    index is never dereferenced and sends no gradient.  Differentiable in x (float atomics: not bit-reproducible where
    an index repeats)."""
    _lib.require_gpu(x, idx)
    if x.dim() != 3 or idx.dim() != 3 or x.shape[0] != idx.shape[0]:
        raise ValueError("knn_gather: x [N,M,U] and idx [N,L,K] expected, got %s and %s" % (tuple(x.shape), tuple(idx.shape)))
    if x.dtype != torch.float32:
        raise ValueError("knn_gather: x must be float32, got %s" % x.dtype)
    if idx.dtype not in (torch.int64, torch.int32):
        raise ValueError("knn_gather: idx must be int64 or int32, got %s" % idx.dtype)
    if 0 in x.shape or 0 in idx.shape:
        raise ValueError("knn_gather: x and idx must not be empty, got %s and %s" % (tuple(x.shape), tuple(idx.shape)))
    return _KnnGather.apply(x, idx, lengths)
