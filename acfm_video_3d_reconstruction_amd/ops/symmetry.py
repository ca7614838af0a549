"""The symmetric template's mirror and its gradient fold (csrc/acfm_deform.hip; template.py is the host side)."""
import torch

from .. import _lib
from .base import _f32c


def _counts(name, t, rows_extra, num_sym):
    """(B, n_indept) of a [rows,3] / [B,rows,3] tensor whose rows are n_indept + num_sym (+ num_sym when rows_extra)."""
    num_sym = int(num_sym)
    if t.dim() not in (2, 3) or t.shape[-1] != 3:
        raise ValueError("%s takes [n,3] or [B,n,3], got %s" % (name, tuple(t.shape)))
    n_indept = t.shape[-2] - num_sym * (2 if rows_extra else 1)
    if num_sym < 0 or n_indept < 0 or t.shape[-2] == 0:
        raise ValueError("%s: num_sym = %d does not fit %d rows (%s)" % (
            name, num_sym, t.shape[-2], "num_indept + 2 num_sym" if rows_extra else "num_indept + num_sym"))
    return (t.shape[0] if t.dim() == 3 else 1), n_indept


class _Symmetrize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, half, num_sym):
        _lib.require_gpu(half)
        B, n_indept = _counts("ops.symmetrize", half, False, num_sym)
        # the tensor goes to the C ABI as it is: a non-contiguous or non-float32 one is refused there, by name
        full = torch.empty(half.shape[:-2] + (half.shape[-2] + num_sym, 3), dtype=torch.float32, device=half.device)
        _lib.call("acfm_symmetrize", half.device, half.detach(), B, n_indept, int(num_sym), full)
        ctx.num_sym = int(num_sym)
        return full

    @staticmethod
    def backward(ctx, g):
        return symmetrize_fold(_f32c(g), ctx.num_sym), None


def symmetrize(V_half, num_sym):
    """MeshNet.symmetrize (mesh_net.py:573-591) in one launch each way: [n_half,3] or [B,n_half,3] ->
    [.., n_half + num_sym, 3], the last num_sym rows appended once more as (-x, y, z)."""
    return _Symmetrize.apply(V_half, num_sym)


def symmetrize_fold(grad_full, num_sym):
    """The backward of symmetrize on its own (no autograd): grad_full [.., n_indept + 2 num_sym, 3] ->
    [.., n_indept + num_sym, 3], the left rows' gradient added to the right rows' with x negated."""
    _lib.require_gpu(grad_full)
    B, n_indept = _counts("ops.symmetrize_fold", grad_full, True, num_sym)
    out = torch.empty(grad_full.shape[:-2] + (grad_full.shape[-2] - num_sym, 3), dtype=torch.float32,
                      device=grad_full.device)
    _lib.call("acfm_symmetrize_backward", grad_full.device, grad_full.detach(), B, n_indept, int(num_sym), out)
    return out
