"""Terms over the hypotheses and frames of a clip: hypothesis total, texture cycle."""
import ctypes

import torch

from .. import _lib
from .base import _f32c


class _HypTotal(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weights, aux_group, aux_weights, G, N, *terms):
        _lib.require_gpu(*terms)
        ts = [_f32c(t).reshape(-1) for t in terms]
        nt = len(ts)
        if not 1 <= nt <= 8 or any(t.numel() != G * N for t in ts) or len(weights) != nt:
            raise ValueError("hypothesis_total: 1..8 terms of G*N elements, one weight each")
        dev = ts[0].device
        total = torch.empty((G, N), dtype=torch.float32, device=dev)
        probs = torch.empty((G, N), dtype=torch.float32, device=dev)
        aux = torch.empty((2, G, N), dtype=torch.float32, device=dev)
        out = torch.empty(12, dtype=torch.float32, device=dev)
        w = (ctypes.c_float * nt)(*[float(x) for x in weights])
        ag = (ctypes.c_int * nt)(*[int(x) for x in aux_group])
        aw = (ctypes.c_float * nt)(*[float(x) for x in aux_weights])
        ptrs = (ctypes.c_void_p * nt)(*[t.data_ptr() for t in ts])
        _lib.call("acfm_hypothesis_total", dev, ptrs, w, ag, aw, nt, G, N, total, probs, aux[0], aux[1], out)
        ctx.args = (w, nt, G, N, [t.shape for t in terms])
        ctx.save_for_backward(probs)
        ctx.mark_non_differentiable(total, probs, aux, out)
        return out[0], total, probs, aux, out

    @staticmethod
    def backward(ctx, go, *_):
        w, nt, G, N, shapes = ctx.args
        probs, = ctx.saved_tensors
        g = _f32c(go).reshape(1)
        need = ctx.needs_input_grad[5:]
        outs = [torch.empty((G, N), dtype=torch.float32, device=g.device) if need[i] else None for i in range(nt)]
        ptrs = (ctypes.c_void_p * nt)(*[(o.data_ptr() if o is not None else None) for o in outs])
        _lib.call("acfm_hypothesis_total_backward", g.device, g, probs, w, nt, G, N, ptrs)
        return (None,) * 5 + tuple(o.reshape(shapes[i]) if o is not None else None for i, o in enumerate(outs))


def hypothesis_total(terms, weights, G, N, aux_group=None, aux_weights=None):
    """Per-hypothesis total, its softmax weighting and the weighted mean (multiframe/main.py:716-746) as one launch
    each way.  terms: 1..8 tensors of G*N elements (row g*N + n); weights: one float each.
    Returns (weighted, total [G,N], probs [G,N], aux [2,G,N], means [12]): weighted = (1/N) sum_n sum_g probs total with
    probs = softmax(-total, dim 0) carrying no gradient; aux[k] = sum of aux_weights[t] * terms[t] over the terms with
    aux_group[t] == k; means = (weighted, mean total, mean aux0, mean aux1, mean of each term ...).  Only `weighted`
    is differentiable."""
    nt = len(terms)
    ag = tuple(aux_group) if aux_group is not None else (-1,) * nt
    aw = tuple(aux_weights) if aux_weights is not None else (0.0,) * nt
    return _HypTotal.apply(tuple(float(w) for w in weights), ag, aw, int(G), int(N), *terms)


class _TexCycle(torch.autograd.Function):
    @staticmethod
    def forward(ctx, textures, T):
        _lib.require_gpu(textures)
        x = _f32c(textures)
        if x.dim() != 5 or x.shape[2] != x.shape[3] or x.shape[4] != 3 or x.shape[0] % int(T) != 0 or x.shape[2] < 2:
            raise ValueError("texture_cycle: atlases [B*T,F,R,R,3] with R >= 2, got %s (T = %d)" % (tuple(x.shape), T))
        B, F, R = x.shape[0] // int(T), x.shape[1], x.shape[2]
        scratch = torch.empty(_lib.lib().acfm_texture_cycle_scratch_floats(B, int(T), F, R), dtype=torch.float32,
                              device=x.device)
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        _lib.call("acfm_texture_cycle", x.device, x, B, int(T), F, R, scratch, loss)
        ctx.save_for_backward(x, scratch)
        ctx.cfg = (B, int(T), F, R, textures.dtype)
        return loss

    @staticmethod
    def backward(ctx, go):
        x, scratch = ctx.saved_tensors
        B, T, F, R, dt = ctx.cfg
        g = _f32c(go).reshape(1)
        gx = torch.empty_like(x)
        _lib.call("acfm_texture_cycle_backward", x.device, x, scratch, g, B, T, F, R, gx)
        return (gx if dt == torch.float32 else gx.to(dt)), None


def texture_cycle(textures, num_frames):
    """The texture temporal-consistency term of ShapeTrainer.forward as written there (multiframe/main.py:705-711):
    atlases [B*T,F,R,R,3] -> scalar; two launches forward, one backward (fixed summation order)."""
    return _TexCycle.apply(textures, int(num_frames))
