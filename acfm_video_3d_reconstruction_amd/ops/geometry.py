"""Projection, deformation (apply and solve) and cameras."""
import ctypes
import math
import weakref

import torch

from .. import _lib
from .base import _LOCK, _f32c


# ------------------------------------------------------------------------------ projection
class _Project(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts, cams, offset_z):
        _lib.require_gpu(verts, cams)
        v, c = _f32c(verts), _f32c(cams)
        N, V, _ = v.shape
        out = torch.empty_like(v)
        _lib.call("acfm_project", v.device, v, c, N, V, float(offset_z), out)
        ctx.save_for_backward(v, c)
        return out

    @staticmethod
    def backward(ctx, g):
        v, c = ctx.saved_tensors
        N, V, _ = v.shape
        g = _f32c(g)
        gv = torch.empty_like(v) if ctx.needs_input_grad[0] else None
        gc = torch.empty_like(c) if ctx.needs_input_grad[1] else None
        _lib.call("acfm_project_backward", v.device, v, c, g, N, V, gv, gc)
        return gv, gc, None


class _ProjectXY(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts, cams, offset_z):
        _lib.require_gpu(verts, cams)
        v, c = _f32c(verts), _f32c(cams)
        N, V, _ = v.shape
        out = torch.empty((N, V, 2), dtype=torch.float32, device=v.device)
        _lib.call("acfm_project_xy", v.device, v, c, N, V, float(offset_z), out)
        ctx.save_for_backward(v, c)
        return out

    @staticmethod
    def backward(ctx, g):
        v, c = ctx.saved_tensors
        N, V, _ = v.shape
        g = _f32c(g)
        gv = torch.empty_like(v) if ctx.needs_input_grad[0] else None
        gc = torch.empty_like(c) if ctx.needs_input_grad[1] else None
        _lib.call("acfm_project_xy_backward", v.device, v, c, g, N, V, gv, gc)
        return gv, gc, None


def project_xy(verts, cams, offset_z=0.0):
    """The (x, y) part of orthographic_proj_withz, [N,V,2]: bit-identical to project(...)[..., :2],
    one launch each way (no slice copy forward, no zero-padded [N,V,3] gradient backward)."""
    return _ProjectXY.apply(verts, cams, offset_z)


def project(verts, cams, offset_z=0.0):
    """[N,V,3] x [N,7] -> [N,V,3]; geom_utils.orthographic_proj_withz semantics."""
    return _Project.apply(verts, cams, offset_z)


# ------------------------------------------------------------------------------ deformation
class _DeformApply(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mean_v, P, delta):
        _lib.require_gpu(mean_v, P, delta)
        m, p, d = _f32c(mean_v), _f32c(P), _f32c(delta)
        N, Kh, _ = d.shape
        V = m.shape[0]
        if p.shape != (V, Kh):
            raise ValueError("P must be [V,K_h] = [%d,%d], got %s" % (V, Kh, tuple(p.shape)))
        out = torch.empty((N, V, 3), dtype=torch.float32, device=m.device)
        _lib.call("acfm_deform_apply", m.device, m, p, d, N, V, Kh, out)
        ctx.save_for_backward(p, d)
        ctx.sink = _sink_entry(P)      # the registration of this very P object, if any (not of its address)
        return out

    @staticmethod
    def backward(ctx, g):
        p, d = ctx.saved_tensors
        N, Kh, _ = d.shape
        V = p.shape[0]
        g = _f32c(g)
        gm = torch.empty((V, 3), dtype=torch.float32, device=g.device) if ctx.needs_input_grad[0] else None
        gp = torch.empty_like(p) if ctx.needs_input_grad[1] else None
        gd = torch.empty_like(d) if ctx.needs_input_grad[2] else None
        _lib.call("acfm_deform_apply_backward", g.device, p, d, g, N, V, Kh, gd, gm, None)
        if gp is not None:
            # dL/dP = sum_n g_n delta_n^T feeds the solve's backward, which amplifies its rounding by the conditioning
            # of the system: summed in double and rounded once (acfm_deform_presolve_sums_f64), so that the value does
            # not depend on how the frames are grouped; a frame-sharded step (sharding.SharedShapeExchange) takes the
            # unrounded doubles for its exchange buffer
            ent = ctx.sink
            sink = ent[1]() if (ent is not None and _PRESOLVE_SINKS.get(ent[2]) is ent) else None   # (still registered)
            if sink is not None:       # (G [V,K_h], sum g [V,3]): float64 views INSIDE the exchange buffer
                g64, m64 = sink.presolve_buffer(V, Kh, g.device)
            else:
                g64, m64 = torch.empty((V, Kh), dtype=torch.float64, device=g.device), None
            _lib.call("acfm_deform_presolve_sums_f64", g.device, d, g, N, V, Kh, g64, m64, gp)
            if sink is not None and hasattr(sink, "presolve_rounded"):
                sink.presolve_rounded(gp, gm)      # (the float32 twins of what the sink now holds in double)
        return gm, gp, gd


# id(P leaf) -> (weak reference to that leaf, weak reference to the object that wants the unrounded double sums of its
# backward, the key): presolve_buffer(V, Kh, device) -> persistent float64 tensors ([V,K_h], [V,3]) it will read after the
# backward.  One entry per live exchange.  Both references are weak -- the table keeps neither the exchange (its float64
# store, its factorisation's graph) nor the leaf alive, and an entry goes when either dies -- and a registration is
# matched on the leaf OBJECT: another tensor on the same address (`P.detach()`, a recycled block) is not routed here.
_PRESOLVE_SINKS = {}


def _forget_sink(key, ref):
    with _LOCK:
        ent = _PRESOLVE_SINKS.get(key)
        if ent is not None and (ent[0] is ref or ent[1] is ref):
            del _PRESOLVE_SINKS[key]


def _sink_entry(P):
    ent = _PRESOLVE_SINKS.get(id(P))
    return ent if (ent is not None and ent[0]() is P) else None


def register_presolve_sink(P, sink, previous_key=None):
    """sharding.SharedShapeExchange.apply(): the backward of deform_apply(., P, .) -- of this tensor object P -- writes
    sum_n g_n delta_n^T in double into sink.presolve_buffer(...).  Neither P nor the sink is kept alive.  -> the key to
    hand back as previous_key next time (or to drop_presolve_sink)."""
    key = id(P)
    gone = lambda ref, key=key: _forget_sink(key, ref)
    with _LOCK:
        if previous_key is not None:
            _PRESOLVE_SINKS.pop(previous_key, None)
        _PRESOLVE_SINKS[key] = (weakref.ref(P, gone), weakref.ref(sink, gone), key)
    return key


def drop_presolve_sink(key):
    with _LOCK:
        _PRESOLVE_SINKS.pop(key, None)


def deform_apply(mean_v, P, delta):
    """verts[n] = mean_v + P @ delta[n]  (mean_v [V,3], P [V,K_h], delta [N,K_h,3])."""
    return _DeformApply.apply(mean_v, P, delta)


SOLVE_INFO_HANDOFF = 0x40000000   # ACFM_SOLVE_INFO_HANDOFF (include/acfm_hip.h)


def decode_solve_info(info):
    """Status word of acfm_deform_solve -> None (ok) or the message of the error it stands for."""
    info = int(info)
    if info == 0:
        return None
    if info & SOLVE_INFO_HANDOFF:
        return ("deform_solve: a hand-off wait of the single-launch factorisation expired (a wave of k_chol_tiles was "
                "starved for > 50 ms, e.g. by time-slicing or side-stream kernels on its CU): P holds NaNs -- run the "
                "solve again")
    return ("deform_solve: L^T L + A^T A is not positive definite (pivot tile starting at row %d)"
            % ((info & (SOLVE_INFO_HANDOFF - 1)) - 1))


# Status words of the solves launched with check=False (DeformSolver's per-step factorisations), copied to pinned host
# memory without blocking: (event, pinned int32).  The next deform_solve / solve_status() call reads those whose copy
# has completed and raises for a failed one -- a step late, but never silently and never with a synchronisation.
_SOLVE_PENDING = []


def solve_status(wait=False):
    """Raise RuntimeError for any earlier deform_solve(check=False) whose status word has arrived and reports a failure
    (a non-positive pivot, an expired hand-off).  wait=True: first wait for the outstanding ones (synchronises)."""
    with _LOCK:
        pending, _SOLVE_PENDING[:] = list(_SOLVE_PENDING), []
    msg, keep = None, []
    for ev, host in pending:
        if wait:
            ev.synchronize()
        if ev.query():
            msg = msg or decode_solve_info(host.item())
        else:
            keep.append((ev, host))
    with _LOCK:
        _SOLVE_PENDING[:0] = keep
    if msg:
        raise RuntimeError(msg + " [reported by an earlier deform_solve(check=False)]")


class _DeformSolve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, L, lbs, check):
        _lib.require_gpu(L, lbs)
        l, b = _f32c(L.detach()), _f32c(lbs)
        V, Kh = b.shape
        if l.shape != (V, V):
            raise ValueError("L must be [V,V] = [%d,%d], got %s" % (V, V, tuple(l.shape)))
        if Kh > 128:
            raise ValueError("at most 128 handles (got %d)" % Kh)
        capturing = torch.cuda.is_current_stream_capturing()
        if not capturing:
            solve_status()
        lib = _lib.lib()
        nbytes = lib.acfm_deform_solve_workspace_bytes(V, Kh)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=b.device)
        P = torch.empty((V, Kh), dtype=torch.float32, device=b.device)
        _lib.call("acfm_deform_solve", b.device, l, b, V, Kh, P, ws, nbytes)
        if check:
            info = ctypes.c_int(0)
            _lib.call("acfm_deform_solve_info", b.device, ws, nbytes, V, ctypes.byref(info))
            msg = decode_solve_info(info.value)
            if msg:
                raise RuntimeError(msg)
        elif not capturing:
            off = lib.acfm_deform_solve_info_offset(V)
            with torch.cuda.device(b.device):
                host = torch.empty(1, dtype=torch.int32, pin_memory=True)
                host.copy_(ws[off:off + 4].view(torch.int32), non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(b.device))
                with _LOCK:
                    _SOLVE_PENDING.append((ev, host))
                    del _SOLVE_PENDING[:-8]
        ctx.ws, ctx.dims = ws, (V, Kh)
        return P

    @staticmethod
    def backward(ctx, g):
        V, Kh = ctx.dims
        if not ctx.needs_input_grad[1]:
            return None, None, None
        g = _f32c(g)
        gl = torch.empty((V, Kh), dtype=torch.float32, device=g.device)
        _lib.call("acfm_deform_solve_backward", g.device, g, V, Kh, ctx.ws, ctx.ws.numel(), gl)
        return None, gl, None


def deform_solve(L, lbs_logits, check=False):
    """P [V,K_h] = (L^T L + A^T A)^-1 A^T with A = softmax(lbs_logits, dim 0)^T: the reference's
    per-frame Cholesky solve (multiframe/main.py:586-609) collapsed to one fp64 factorisation per
    step.  L [V,V] dense Laplacian (no gradient), lbs_logits [V,K_h] (gradient supported), K_h <= 128 (the
    reference's 64-handle bird model and its 128-handle default; ValueError beyond) and V <= 16384.  Up to 32
    handles are one panel of right-hand sides; every further 32 add a panel of tile jobs to the same launch.
    check=True synchronises and raises if the matrix is not positive definite or a hand-off of the single-launch
    factorisation timed out (decode_solve_info); check=False (the per-step path) copies the status word to the host
    without blocking and the NEXT deform_solve / solve_status() call raises for it."""
    return _DeformSolve.apply(L, lbs_logits, bool(check))


# ------------------------------------------------------------------------------ cameras
# The two embeddings -- (scale, trans, quaternion), 7 floats, and the (scale, trans, azimuth, elevation, cyclo-rotation)
# of --az_el_cam, 6 floats -- share these bindings: `entry` names the C entry point (its backward is entry + "_backward"),
# W the embedding width, params the decode parameters the entry point takes after (R, N).
class _CameraPipeline(torch.autograd.Function):
    @staticmethod
    def forward(ctx, emb, mirror_flag, transforms, entry, W, params):
        _lib.require_gpu(emb, mirror_flag, transforms)
        e = _f32c(emb)
        R = e.numel() // W
        mf = mirror_flag.detach().reshape(-1).to(torch.int64).contiguous()
        tr = _f32c(transforms).reshape(-1, 4)
        N = mf.numel()
        if tr.shape[0] != N or R % N != 0:
            raise ValueError("camera rows %d must be a multiple of the %d frames (transforms %s)"
                             % (R, N, tuple(tr.shape)))
        out = torch.empty((R, 7), dtype=torch.float32, device=e.device)
        _lib.call(entry, e.device, e, mf, tr, R, N, *params, out)
        ctx.save_for_backward(e, mf, tr)
        ctx.cfg = (entry, W, params)
        return out

    @staticmethod
    def backward(ctx, g):
        e, mf, tr = ctx.saved_tensors
        entry, W, params = ctx.cfg
        R, N = e.numel() // W, mf.numel()
        g = _f32c(g)
        ge = torch.empty_like(e)
        _lib.call(entry + "_backward", e.device, e, mf, tr, g, R, N, *params, ge)
        return ge, None, None, None, None, None


def camera_pipeline(cam_emb, mirror_flag, transforms, scale_lr_decay=1.0):
    """Camera embeddings [G,N,7] (or [R,7], row r of frame r % N) -> cameras [R,7]: decode, mirror by
    the per-frame flag [N], crop/scale transform [N,4] (multiframe/main.py:551-584) in one kernel."""
    return _CameraPipeline.apply(cam_emb, mirror_flag, transforms, "acfm_camera_pipeline", 7, (float(scale_lr_decay),))


def _azel_params(scale_lr_decay, scale_bias, euler_range_deg):
    """-> (decay, bias, az, el, cyc) as the kernels take them: the three ranges converted to radians, once, here."""
    rng = tuple(float(d) for d in euler_range_deg)
    if len(rng) != 3:
        raise ValueError("euler_range_deg must be (az, el, cyc) in degrees, got %r" % (euler_range_deg,))
    return (float(scale_lr_decay), float(scale_bias)) + tuple(math.pi / 180 * d for d in rng)


def camera_pipeline_azel(cam_emb, mirror_flag, transforms, scale_lr_decay=0.05, scale_bias=1.0,
                         euler_range_deg=(30., 60., 60.)):
    """Az/el camera embeddings [G,N,6] (or [R,6], row r of frame r % N; columns scale, tx, ty, azimuth, elevation,
    cyclo-rotation) -> cameras [R,7]: the decode of --az_el_cam (multiframe/main.py:554-566, mesh_net.py:310-385:
    s = decay*e0 + bias, q = q_cyc (x) q_el (x) q_az from the angles (range*e3, pi - range*e4, range*e5)), then the
    mirror and the crop/scale transform of camera_pipeline, in one kernel each way.  euler_range_deg = (az, el, cyc) in
    degrees, as the reference's --az_euler_range / --el_euler_range / --cyc_euler_range are."""
    return _CameraPipeline.apply(cam_emb, mirror_flag, transforms, "acfm_camera_pipeline_azel", 6,
                                 _azel_params(scale_lr_decay, scale_bias, euler_range_deg))


class _CameraPipelineTables(torch.autograd.Function):
    @staticmethod
    def forward(ctx, frames_idx, selected, mirror_flag, transforms, entry, W, params, G, *tables):
        _lib.require_gpu(frames_idx, mirror_flag, transforms, *tables)
        what = entry[5:]
        ts = [_f32c(t) for t in tables]
        F = ts[0].shape[0]
        if not 1 <= len(ts) <= 32 or any(t.dim() != 2 or tuple(t.shape) != (F, W) for t in ts):
            raise ValueError("%s: 1..32 embedding tables [frames, %d] of one size" % (what, W))
        fi = frames_idx.detach().reshape(-1).to(torch.int64).contiguous()
        mf = mirror_flag.detach().reshape(-1).to(torch.int64).contiguous()
        tr = _f32c(transforms).reshape(-1, 4)
        N = fi.numel()
        R = int(G) * N
        sel = None if selected is None else selected.detach().reshape(-1).to(torch.int64).contiguous()
        if mf.numel() != N or tr.shape[0] != N or (sel is not None and sel.numel() != R) or \
                (sel is None and int(G) > len(ts)):
            raise ValueError("%s: %d frames, mirror flags %d, transforms %s, G = %d, %d tables"
                             % (what, N, mf.numel(), tuple(tr.shape), G, len(ts)))
        out = torch.empty((R, 7), dtype=torch.float32, device=ts[0].device)
        ptrs = (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        _lib.call(entry, out.device, ptrs, len(ts), F, fi, sel, mf, tr, R, N, *params, out)
        ctx.save_for_backward(fi, mf, tr, *ts) if sel is None else ctx.save_for_backward(fi, mf, tr, sel, *ts)
        ctx.cfg = (entry, W, params, R, N, F, len(ts), sel is not None)
        return out

    @staticmethod
    def backward(ctx, g):
        entry, W, params, R, N, F, nt, has_sel = ctx.cfg
        saved = ctx.saved_tensors
        fi, mf, tr = saved[:3]
        sel = saved[3] if has_sel else None
        ts = saved[4:] if has_sel else saved[3:]
        g = _f32c(g)
        need = ctx.needs_input_grad[8:]
        outs = [torch.empty((F, W), dtype=torch.float32, device=g.device) if need[i] else None for i in range(nt)]
        ptrs = (ctypes.c_void_p * nt)(*[t.data_ptr() for t in ts])
        gptrs = (ctypes.c_void_p * nt)(*[(o.data_ptr() if o is not None else None) for o in outs])
        _lib.call(entry + "_backward", g.device, ptrs, nt, F, fi, sel, mf, tr, g, R, N, *params, gptrs)
        return (None,) * 8 + tuple(outs)


def _check_table_ids(what, tables, frames_idx, selected):
    nf = tables[0].shape[0]
    lo, hi = int(frames_idx.min()), int(frames_idx.max())
    if lo < 0 or hi >= nf:
        raise IndexError("%s: frames_idx in [%d, %d] outside the %d rows of the embedding tables" % (what, lo, hi, nf))
    if selected is not None and (int(selected.min()) < 0 or int(selected.max()) >= len(tables)):
        raise IndexError("%s: selected hypothesis outside the %d tables" % (what, len(tables)))


def camera_pipeline_tables(tables, frames_idx, mirror_flag, transforms, scale_lr_decay=1.0, num_guesses=None,
                           selected=None, check=False):
    """Cameras [G*N,7] of all hypotheses straight from the per-hypothesis embedding tables ([frames,7] each,
    mesh_net.py:436-444): the look-ups, the stack / top-k gather (main.py:551-570) and the decode / mirror / transform
    chain (:572-584) in one kernel each way.  Row g*N + n reads tables[selected[g, n] if given else g][frames_idx[n]];
    the backward returns dense [frames,7] gradients like nn.Embedding's.
    A frames_idx outside [0, frames) or a `selected` outside [0, len(tables)) -- where nn.Embedding raises -- gives that
    row a NaN camera and no gradient (never an out-of-bounds access); check=True validates both on the host first
    (one synchronisation: for data-loader batches, not inside a captured step) and raises IndexError."""
    G = len(tables) if num_guesses is None else int(num_guesses)
    if check:
        _check_table_ids("camera_pipeline_tables", tables, frames_idx, selected)
    return _CameraPipelineTables.apply(frames_idx, selected, mirror_flag, transforms, "acfm_camera_pipeline_tables", 7,
                                       (float(scale_lr_decay),), G, *tables)


def camera_pipeline_azel_tables(tables, frames_idx, mirror_flag, transforms, scale_lr_decay=0.05, scale_bias=1.0,
                                euler_range_deg=(30., 60., 60.), num_guesses=None, selected=None, check=False):
    """camera_pipeline_tables for the az/el embedding tables ([frames,6] each, mesh_net.py:405-416): the look-ups, the
    stack / top-k gather and the camera_pipeline_azel chain in one kernel each way.  Row g*N + n reads
    tables[selected[g, n] if given else g][frames_idx[n]]; the backward returns dense [frames,6] gradients, every cell
    summed in a fixed order.  Out-of-range frames_idx / selected give that row a NaN camera and no gradient (never an
    out-of-bounds access); check=True validates both on the host first (one synchronisation) and raises IndexError."""
    G = len(tables) if num_guesses is None else int(num_guesses)
    if check:
        _check_table_ids("camera_pipeline_azel_tables", tables, frames_idx, selected)
    return _CameraPipelineTables.apply(frames_idx, selected, mirror_flag, transforms, "acfm_camera_pipeline_azel_tables",
                                       6, _azel_params(scale_lr_decay, scale_bias, euler_range_deg), G, *tables)


def camera_mirror(cams):
    """Decoded cameras [R,7] -> the pose of the horizontally flipped image (multiframe/main.py:97-125 with the flag
    set), one kernel; no gradient (the texture render it feeds sends none to its cameras)."""
    _lib.require_gpu(cams)
    c = _f32c(cams.detach()).reshape(-1, 7)
    out = torch.empty_like(c)
    _lib.call("acfm_camera_mirror", c.device, c, c.shape[0], out)
    return out


class _CameraNormalize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, raw):
        _lib.require_gpu(raw)
        r = _f32c(raw)
        N = r.numel() // 7
        out = torch.empty_like(r)
        _lib.call("acfm_camera_normalize", r.device, r, N, out)
        ctx.save_for_backward(r)
        return out

    @staticmethod
    def backward(ctx, g):
        (r,) = ctx.saved_tensors
        g = _f32c(g)
        gr = torch.empty_like(r)
        _lib.call("acfm_camera_normalize_backward", r.device, r, g, r.numel() // 7, gr)
        return gr


def camera_normalize(cam_raw):
    """[N,7] (s, tx, ty, q) -> (s, tx, ty, q/|q|): torch.cat([scale, trans, F.normalize(quat)]) in one kernel."""
    return _CameraNormalize.apply(cam_raw)
