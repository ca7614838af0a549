"""The loss operators of a step that defer their launch: mask_losses, tex_mse, bds_loss_per_mesh, combine_losses."""
import ctypes

import torch

from .. import _lib
from .base import (LAZY_GRADS, LazyGrad, _LOSS_BDS, _LOSS_MASK, _LOSS_TEX_MSE, _capture_id, _f32c, _loss_scratch,
                   _ref_batch)
from .pending import PendingTerm, _PendingJob, _deferring, _launch_step_tail, _raw


# ------------------------------------------------------------------------------ mask losses
class _MaskLosses(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mask, gt, edt):
        _lib.require_gpu(mask, gt, edt)
        m = _f32c(mask)
        N = m.shape[0]
        HW = m[0].numel()
        g = _f32c(gt).reshape(-1, HW) if gt is not None else None
        e = _f32c(edt).reshape(-1, HW) if edt is not None else None
        RB = N
        for r in (g, e):
            if r is not None:
                RB = _ref_batch(N, r, "mask_losses")
        if g is not None and e is not None and g.shape[0] != e.shape[0]:
            raise ValueError("mask_losses: gt and edt must have the same batch")
        out = torch.empty((N, 4), dtype=torch.float32, device=m.device)

        def launch():
            with torch.cuda.device(m.device):
                tk, part, nf = _loss_scratch(m.device, _LOSS_MASK, N, HW)
            _lib.call("acfm_mask_losses", m.device, m, g, e, N, HW, RB, out, tk, part, nf)
        ctx.save_for_backward(m, g, e)
        ctx.rb = RB
        ctx.job = None
        if not _deferring(m.device, "mask"):
            launch()
            return out
        ctx.job = _PendingJob(
            "mask", "mask_losses", out, N, (("mask", m), ("gt", g), ("edt", e)), launch,
            lambda: _lib.StepMaskJob(m.data_ptr(), g.data_ptr() if g is not None else None,
                                     e.data_ptr() if e is not None else None, out.data_ptr(), HW, RB), HW)
        return PendingTerm(out, ctx.job)

    @staticmethod
    def backward(ctx, gout):
        if ctx.job is not None:
            ctx.job.flush()
        m, g, e = ctx.saved_tensors
        N = m.shape[0]
        HW = m[0].numel()
        go = _f32c(gout)
        rb = ctx.rb

        def make():
            gm = torch.empty_like(m)
            _lib.call("acfm_mask_losses_backward", m.device, m, g, e, go, N, HW, rb, gm)
            return gm
        if LAZY_GRADS[0] and m.dim() >= 2:
            return LazyGrad(m, "mask_losses", (m, g, e, rb, go), make), None, None
        return make(), None, None


def mask_losses(mask, gt=None, edt=None):
    """One pass over the mask -> [N,4] = (mean|m-gt|, sum m*gt, sum(m+gt-m*gt), mean edt*m).
    gt / edt: [N,...] or [N/G,...] shared by G hypotheses per frame (see _ref_batch)."""
    return _MaskLosses.apply(mask, gt, edt)


class _TexMSE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tex, img, mask):
        _lib.require_gpu(tex, img, mask)
        t, i, m = _f32c(tex), _f32c(img), _f32c(mask)
        N = t.shape[0]
        HW = m[0].numel()
        RB = _ref_batch(N, i, "tex_mse")
        if t.shape[1:] != i.shape[1:] or t.shape[1] != 3 or t[0, 0].numel() != HW or m.shape[0] != RB:
            raise ValueError("tex [N,3,H,W], img [N or N/G,3,H,W] and mask [same batch as img,H,W]")
        out = torch.empty((N,), dtype=torch.float32, device=t.device)

        def launch():
            with torch.cuda.device(t.device):
                tk, part, nf = _loss_scratch(t.device, _LOSS_TEX_MSE, N, HW)
            _lib.call("acfm_tex_mse", t.device, t, i, m, N, HW, RB, out, tk, part, nf)
        ctx.save_for_backward(t, i, m)
        ctx.rb = RB
        ctx.job = None
        if not _deferring(t.device, "tex"):
            launch()
            return out
        ctx.job = _PendingJob("tex", "tex_mse", out, N, (("tex", t), ("img", i), ("mask", m)), launch,
                              lambda: _lib.StepTexJob(t.data_ptr(), i.data_ptr(), m.data_ptr(), out.data_ptr(), HW, RB),
                              HW)
        return PendingTerm(out, ctx.job)

    @staticmethod
    def backward(ctx, go):
        if ctx.job is not None:
            ctx.job.flush()
        t, i, m = ctx.saved_tensors
        N = t.shape[0]
        HW = m[0].numel()
        g = _f32c(go)
        rb = ctx.rb

        def make():
            gt = torch.empty_like(t)
            _lib.call("acfm_tex_mse_backward", t.device, t, i, m, g, N, HW, rb, gt)
            return gt
        if LAZY_GRADS[0]:
            return LazyGrad(t, "tex_mse", (t, i, m, rb, g), make), None, None
        return make(), None, None


def tex_mse(tex, img, mask):
    """mean over (3,H,W) of (tex*mask - img*mask)^2 per mesh -> [N]; gradient to tex only."""
    return _TexMSE.apply(tex, img, mask)


# ------------------------------------------------------------------------------ loss combination
class _Combine(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weights, *terms):
        _lib.require_gpu(*terms)
        # the terms whose launch is still pending leave with the total, as one launch: at most one of each kind, all
        # called on this stream and in this capture (any other pending term is launched by itself, here)
        jobs = []
        for t in terms:
            j = t._job if type(t) is PendingTerm else None
            if j is not None and not j.done and j not in jobs and all(k.kind != j.kind for k in jobs) and \
                    j.N == terms[0].shape[0] and j.device == terms[0].device and \
                    j.stream == torch.cuda.current_stream(j.device) and j.cid == _capture_id(j.device):
                jobs.append(j)
        fused = {id(j.out) for j in jobs}
        ts = []
        for t in terms:
            r = _raw(t)
            if id(r) in fused:
                ts.append(r if r.dim() == 2 else r.view(r.shape[0], -1))
            else:
                ts.append(_f32c(t if t.dim() == 2 else t.reshape(t.shape[0], -1)))
        N = ts[0].shape[0]
        cols = [int(t.shape[1]) for t in ts]
        if not 1 <= len(ts) <= 4 or any(t.shape[0] != N for t in ts) or any(c < 1 or c > 4 for c in cols) \
                or sum(cols) != len(weights):
            raise ValueError("combine_losses: up to 4 terms [N] or [N,C<=4] with one weight per column")
        total = torch.empty((), dtype=torch.float32, device=ts[0].device)
        ctx.args = ((ctypes.c_int * len(cols))(*cols), (ctypes.c_float * len(weights))(*[float(w) for w in weights]),
                    len(ts), N, [t.shape for t in terms])
        if jobs:
            _launch_step_tail(jobs, (ts, ctx.args[0], ctx.args[1], total))
            return total
        ptrs = (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        _lib.call("acfm_combine_losses", total.device, ptrs, ctx.args[0], ctx.args[1], len(ts), N, total)
        return total

    @staticmethod
    def backward(ctx, go):
        cols, w, nt, N, shapes = ctx.args
        g = _f32c(go).reshape(1)
        need = ctx.needs_input_grad[1:]
        outs = [torch.empty((N, cols[i]), dtype=torch.float32, device=g.device) if need[i] else None
                for i in range(nt)]
        ptrs = (ctypes.c_void_p * nt)(*[(o.data_ptr() if o is not None else None) for o in outs])
        _lib.call("acfm_combine_losses_backward", g.device, g, ptrs, cols, w, nt, N)
        return (None,) + tuple(o.reshape(shapes[i]) if o is not None else None for i, o in enumerate(outs))


def combine_losses(terms, weights):
    """(1/N) sum_n sum_t sum_c w[t][c] * terms[t][n, c] -> scalar: the weighted total of per-mesh loss
    vectors and its batch mean (multiframe/main.py:716-765) as one launch each way.  terms: up to 4
    tensors [N] or [N, C<=4] (e.g. the [N,4] output of mask_losses as it is); weights: one float per
    column, flattened term by term."""
    return _Combine.apply(tuple(float(w) for w in weights), *terms)


# ------------------------------------------------------------------------------ boundary loss
class _BdsLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts_xy, bds, vis):
        _lib.require_gpu(verts_xy, bds, vis)
        v, b = _f32c(verts_xy), _f32c(bds)
        N, V, _ = v.shape
        P = b.shape[1]
        RB = _ref_batch(N, b, "bds_loss")
        loss = torch.empty((N,), dtype=torch.float32, device=v.device)
        arg = torch.empty((N, P), dtype=torch.int32, device=v.device)
        vz = vis.contiguous()

        def launch():
            with torch.cuda.device(v.device):
                tk, part, nf = _loss_scratch(v.device, _LOSS_BDS, N, P)
            _lib.call("acfm_bds_loss", v.device, v, b, vz, None, N, V, P, RB, 0, 0, loss, arg, tk, part, nf)
        ctx.rb = RB
        ctx.job = None
        if not _deferring(v.device, "bds") or 12 * V > 150 * 1024:     # (a V the kernel refuses is refused here, by its own launch)
            ctx.save_for_backward(v, b, arg)
            launch()
            return loss
        ctx.job = _PendingJob("bds", "bds_loss", loss, N, (("verts", v), ("bds", b), ("vis", vz)), launch,
                              lambda: _lib.StepBdsJob(v.data_ptr(), b.data_ptr(), vz.data_ptr(), None, loss.data_ptr(),
                                                      arg.data_ptr(), V, P, RB, 0, 0), P)
        ctx.save_for_backward(v, b, PendingTerm(arg, ctx.job))   # (whoever reads the saved argmin launches the job too)
        return PendingTerm(loss, ctx.job)

    @staticmethod
    def backward(ctx, gl):
        if ctx.job is not None:
            ctx.job.flush()
        v, b, arg = ctx.saved_tensors
        N, V, _ = v.shape
        P = b.shape[1]
        g = _f32c(gl)
        gv = torch.empty_like(v)
        _lib.call("acfm_bds_loss_backward", v.device, v, b, None, arg, g, N, V, P, ctx.rb, 0, 0, gv)
        return gv, None, None


class _BdsLossSel(torch.autograd.Function):
    """_BdsLoss with every point read through a slot list (acfm_bds_loss with sel): no gathered copy of the points."""

    @staticmethod
    def forward(ctx, verts_xy, bds, vis, sel):
        _lib.require_gpu(verts_xy, bds, vis, sel)
        v, b = _f32c(verts_xy), _f32c(bds)
        N, V, _ = v.shape
        P = b.shape[1]
        RB = _ref_batch(N, b, "bds_loss")
        if sel.dtype != torch.int32 or sel.dim() != 2 or sel.shape[0] not in (1, RB):
            raise ValueError("bds_loss: sel must be int32 [1, S] or [%d, S], got %s %s"
                             % (RB, sel.dtype, tuple(sel.shape)))
        s = sel.contiguous()
        rows, S = s.shape
        loss = torch.empty((N,), dtype=torch.float32, device=v.device)
        arg = torch.empty((N, S), dtype=torch.int32, device=v.device)
        vz = vis.contiguous()

        def launch():
            with torch.cuda.device(v.device):
                tk, part, nf = _loss_scratch(v.device, _LOSS_BDS, N, S)
            _lib.call("acfm_bds_loss", v.device, v, b, vz, s, N, V, P, RB, rows, S, loss, arg, tk, part, nf)
        ctx.rb = RB
        ctx.job = None
        if not _deferring(v.device, "bds") or 12 * V > 150 * 1024:
            ctx.save_for_backward(v, b, s, arg)
            launch()
            return loss
        ctx.job = _PendingJob("bds", "bds_loss", loss, N, (("verts", v), ("bds", b), ("vis", vz), ("sel", s)), launch,
                              lambda: _lib.StepBdsJob(v.data_ptr(), b.data_ptr(), vz.data_ptr(), s.data_ptr(),
                                                      loss.data_ptr(), arg.data_ptr(), V, P, RB, rows, S), S)
        ctx.save_for_backward(v, b, s, PendingTerm(arg, ctx.job))
        return PendingTerm(loss, ctx.job)

    @staticmethod
    def backward(ctx, gl):
        if ctx.job is not None:
            ctx.job.flush()
        v, b, s, arg = ctx.saved_tensors
        N, V, _ = v.shape
        P = b.shape[1]
        rows, S = s.shape
        g = _f32c(gl)
        gv = torch.empty_like(v)
        _lib.call("acfm_bds_loss_backward", v.device, v, b, s, arg, g, N, V, P, ctx.rb, rows, S, gv)
        return gv, None, None, None


def bds_loss_per_mesh(verts_xy, bds, vis, sel=None):
    """[N,V,2] x [N,P,3] x uint8 [N,V] -> [N] (sum over boundary points).
    sel (int32 [1,S] or [RB,S], from boundary_subset): only the points whose slots it names are summed, -1 entries
    are skipped; the points are read in place."""
    if sel is None:
        return _BdsLoss.apply(verts_xy, bds, vis)
    return _BdsLossSel.apply(verts_xy, bds, vis, sel)


def boundary_subset(state, P, n_samples, counts=None, per_mesh=False):
    """The draw of loss_utils.bds_loss (:211, torch.randperm(P)[:n_samples]) on the device -> sel int32
    [rows, n_samples]: per row a uniform random subset of min(n_samples, P_r) of the slots [0, P_r) in ascending
    order, then -1.  state: int64 [2] = (seed, draw) on the GPU; the call uses draw = state[1] and advances it by one
    in stream order (no host synchronisation: a captured call draws afresh at every replay).  counts: int32 [RB] true
    list lengths, or None.  per_mesh=False: one row for the batch, P_0 = min(P, max(counts)) (the reference's one
    subset over the padded length when counts is None); per_mesh=True: rows = RB, P_r = min(P, counts[r]).
    The draws have the reference's distribution, not its random stream; boundary_sampling.subset_host is the
    definition, index for index."""
    _lib.require_gpu(state, counts)
    if state.dtype != torch.int64 or tuple(state.shape) != (2,) or not state.is_contiguous():
        raise ValueError("boundary_subset: state must be a contiguous int64 [2] tensor (seed, draw)")
    if per_mesh and counts is None:
        raise ValueError("boundary_subset: per_mesh=True needs counts")
    nc = 0
    if counts is not None:
        if counts.dtype != torch.int32 or counts.dim() != 1 or counts.device != state.device:
            raise ValueError("boundary_subset: counts must be int32 [RB] on the state's device")
        counts = counts.contiguous()
        nc = counts.shape[0]
    rows = nc if per_mesh else 1
    sel = torch.empty((rows, int(n_samples)), dtype=torch.int32, device=state.device)
    _lib.call("acfm_boundary_subset", state.device, state, counts, nc, rows, int(P), int(n_samples), sel)
    return sel
