"""torch.autograd bindings of the C ABI (include/acfm_hip.h).

torch is used here for device memory, streams and autograd bookkeeping only; every op body
is one or more stream-ordered calls into libacfm_hip.so."""
import contextlib
import ctypes
import dataclasses
import math
import threading
import weakref

import torch

from . import _lib

SIL_K = 20  # nmr.py:158
SIL_SIGMA = 1e-4  # nmr.py:153
SIL_BLUR = math.log(1.0 / 1e-4 - 1.0) * 1e-4  # nmr.py:157


def _f32c(t):
    if type(t) is LazyGrad:          # (defined below) a gradient another operator of this module has not formed yet
        t = t.materialize()
    return t.detach().to(torch.float32).contiguous()


def _real(t, f16):
    """Storage tensor of the raster ops: float32, or float16 with storage="f16" (ACFM_STORE_F16)."""
    return t.detach().to(torch.float16 if f16 else torch.float32).contiguous()


def _is_f16(storage):
    if storage not in ("f32", "f16"):
        raise ValueError("storage must be 'f32' or 'f16', got %r" % (storage,))
    return storage == "f16"


_FACES = {}   # (storage ptr, offset, strides, version, shape, N) -> (source kept alive, contiguous int64 [N,F,3])


def expand_faces(faces, N):
    """faces [F,3] / [1,F,3] / [N,F,3] -> contiguous int64 [N,F,3] on the same device.  The
    reference passes one face list broadcast over the batch (`faces[None].expand(N, -1, -1)`) to
    every render call; its materialised copy is memoised on the source tensor (storage, version)."""
    if faces.dim() == 2:
        faces = faces[None]
    if faces.shape[0] != N:
        if faces.shape[0] != 1:
            raise ValueError("faces batch %d does not match %d meshes" % (faces.shape[0], N))
        faces = faces.expand(N, -1, -1)
    if faces.dtype == torch.int64 and faces.is_contiguous():
        return faces
    key = (faces.data_ptr(), faces.storage_offset(), faces.stride(), faces._version, tuple(faces.shape),
           str(faces.dtype), str(faces.device))
    with _LOCK:
        hit = _FACES.get(key)
        if hit is None:
            if len(_FACES) > 8:
                _FACES.clear()
            hit = _FACES[key] = (faces, faces.to(torch.int64).contiguous())
    return hit[1]


def _workspace(N, V, F, H, device):
    nbytes = _lib.lib().acfm_raster_workspace_bytes(N, V, F, H)
    return torch.empty(nbytes, dtype=torch.uint8, device=device), nbytes


# The face setup (projection, face records, coarse masks, schedule) of the last silhouette render
# per device.  The reference renders the texture of the same prediction right after its silhouette
# (multiframe/main.py:616-636): when verts / cams / faces are the same storage at the same version,
# the texture render takes the workspace over instead of setting up again (acfm_tex_forward,
# ws_ready).  The entry keeps its tensors alive, so an address cannot be recycled under it.
#
# What makes a take-over safe -- all of it is part of the key:
#   * same tensors: storage address, shape and autograd version of verts / cams / faces;
#   * same HIP stream (the texture render is ordered behind the silhouette render that filled ws);
#   * same capture: both calls are eager, or both are recorded into the SAME hipGraph capture (id from
#     hipStreamGetCaptureInfo) -- a workspace never crosses a graph boundary;
#   * same epoch: invalidate_setups() ends every sharing.  A hipGraph REPLAY rewrites the tensors its capture wrote
#     without touching their version counters, so whoever replays a graph and then hands such tensors to the renderers
#     eagerly announces it with invalidate_setups() (graphed.GraphedStep.replay and bench.py do; torch itself is not
#     edited -- round 2 wrapped torch.cuda.CUDAGraph.replay process-wide for this).  Writes that bypass the version
#     counters in other ways (`t.data` in-place ops, foreign kernels on raw pointers) are the caller's to announce
#     the same way; share_setup(False) turns the take-over off.
# The caches below (_SETUP, _COVER, _FACES) are shared by the threads nn.DataParallel runs its replicas on
# (main.py:183-193): every read-modify-write of them happens under _LOCK.
_SETUP = {}
_EPOCH = [0]
_SHARE = [True]
_LOCK = threading.RLock()


def invalidate_setups():
    """Forget every cached face setup: call after writing to verts / cams / faces behind torch's back, and after a
    hipGraph replay whose outputs are then rendered eagerly (see above)."""
    flush_pending_losses()    # (a replay rewrites the inputs a deferred loss term has yet to read)
    with _LOCK:
        _EPOCH[0] += 1
        _SETUP.clear()


def share_setup(on):
    """Enable / disable the silhouette -> texture workspace take-over (default on).  Returns the old value."""
    with _LOCK:
        old, _SHARE[0] = _SHARE[0], bool(on)
        if not on:
            _SETUP.clear()
    return old


def graph_replay(graph):
    """graph.replay() + invalidate_setups(): the replay of a torch.cuda.CUDAGraph whose tensors are also handed to
    the renderers outside the graph."""
    invalidate_setups()
    return graph.replay()


def _capture_id(device):
    """0 when the current stream of `device` is not capturing, else the id of the capture."""
    if not torch.cuda.is_current_stream_capturing():
        return 0
    cid = ctypes.c_ulonglong(0)
    _lib.check(_lib.lib().acfm_stream_capture_id(_lib.cur_stream(device), ctypes.byref(cid)), "acfm_stream_capture_id")
    return int(cid.value) or -1


def _setup_key(v, c, f, H, offset_z):
    return (v.data_ptr(), v._version, tuple(v.shape), c.data_ptr(), c._version, f.data_ptr(), f._version,
            tuple(f.shape), int(H), float(offset_z), torch.cuda.current_stream(v.device).cuda_stream,
            _capture_id(v.device), _EPOCH[0])


# Scratch of the one-launch loss sums (acfm_mask_losses_ws, acfm_tex_mse_ws, acfm_bds_loss_ws: include/acfm_hip.h):
# per (device, stream, capture, loss) one ticket word per mesh -- zero before the first launch, left at zero by
# every launch -- and a buffer for the workgroups' partial sums (any contents).  Keyed like that, two calls that can
# be in flight at the same time never share them, and a captured graph keeps the addresses it was recorded with.
#   * The ticket words are slices (N rounded up to 64 words) of zeroed 256 KiB chunks, so handing one out launches
#     nothing -- inside a capture a fill would be recorded and replayed with every step.  A spent chunk is followed
#     by a new one; only if that has to happen inside a capture (first use on the device, or chunk spent there) are
#     the words a zeroed tensor of their own, whose fill the graph then replays: call a loss once eagerly first.
#   * Reclaiming: an eager entry lives as long as its stream is used (a bigger call replaces it).  A capture's entry
#     (64 words and a few KiB per loss at 64 meshes) is kept, because the graph may be replayed at any time;
#     reset_loss_scratch() drops everything once no such graph is left.
#   * A launch that is killed midway (device fault, abort) leaves its ticket words non-zero, and later sums on them
#     would be wrong without a sign: after any device error call reset_loss_scratch(); loss_tickets_clean() checks.
_TICKET_CHUNKS = {}      # device index -> [int32 tensor, words handed out] (the current chunk)
_LOSS_SCRATCH = {}       # (device index, stream, capture id, which) -> [tickets slice, partials]
_TICKET_CHUNK_WORDS = 1 << 16
_LOSS_MASK, _LOSS_TEX_MSE, _LOSS_BDS = 0, 1, 2
_LOSS_CHAMFER, _LOSS_EDGE_LEN, _LOSS_NORMAL = "chamfer", "edge_len", "normal"   # keys only: sized by their own queries


def _ticket_words(device, n, capturing):
    chunk = _TICKET_CHUNKS.get(device.index)
    if (chunk is None or chunk[1] + n > chunk[0].numel()) and not capturing and n <= _TICKET_CHUNK_WORDS:
        chunk = _TICKET_CHUNKS[device.index] = [torch.zeros(_TICKET_CHUNK_WORDS, dtype=torch.int32, device=device), 0]
        torch.cuda.current_stream(device).synchronize()   # once per chunk: its slices are used on any stream
    if chunk is not None and chunk[1] + n <= chunk[0].numel():
        t = chunk[0][chunk[1]:chunk[1] + n]
        chunk[1] += n
        return t
    return torch.zeros(n, dtype=torch.int32, device=device)


def _loss_scratch(device, which, N, n):
    """-> (tickets, partials, floats in partials) for an acfm_*_ws call of loss `which` on the current stream."""
    return _row_scratch(device, which, N, int(_lib.lib().acfm_loss_partial_floats(which, N, n)))


def _row_scratch(device, which, N, need):
    """The same for any kernel with a ticket finish: N ticket words and `need` floats under the key `which`."""
    cid = _capture_id(device)
    key = (device.index, torch.cuda.current_stream(device).cuda_stream, cid, which)
    with _LOCK:
        ent = _LOSS_SCRATCH.get(key)
        if ent is None:
            ent = _LOSS_SCRATCH[key] = [None, None]
        if ent[0] is None or ent[0].numel() < N:
            ent[0] = _ticket_words(device, -(-N // 64) * 64, cid != 0)
        if ent[1] is None or ent[1].numel() < need:
            ent[1] = torch.empty(need, dtype=torch.float32, device=device)
    return ent[0], ent[1], ent[1].numel()


def reset_loss_scratch():
    """Forget the scratch of the one-launch loss sums (fresh, zeroed ticket words on the next call).  For after a
    device error, and to release what captured graphs held once none of them will be replayed again."""
    with _LOCK:
        _LOSS_SCRATCH.clear()
        _TICKET_CHUNKS.clear()


def loss_tickets_clean():
    """Debug check (synchronises): True if every ticket word handed out so far reads zero, as it must whenever no
    loss launch is in flight."""
    with _LOCK:
        held = [e[0] for e in _LOSS_SCRATCH.values() if e[0] is not None]
    torch.cuda.synchronize()
    return all(int(t.abs().max()) == 0 for t in held)


PREFILL_TEX = [True]    # the silhouette render pre-fills the following texture render's empty blocks (see _SilRender.forward)


# ACFM_RECORD_COVER: the silhouette render can note the nearest COVERING face of every pixel on its way (a few
# instructions per covering pair), and the texture render that takes its workspace over then shades from that plane
# instead of binning and walking the faces again (70 -> ~30 us per 64 frames @256^2).  Worth it only when a texture
# render does follow, which the renderer cannot know: per device, the flag is on while the previous silhouette
# render's plane was used, and goes off when a plane was left unread.  Pure speed: outputs are bit-identical.
_COVER = {}


def _cover_tuning(device, tune):
    """Tuning for a silhouette render on `device`: `tune` with the cover flag decided."""
    forced = getattr(tune, "record_cover", None) if tune is not None else None
    if forced is not None:
        return _lib.with_cover(tune, bool(forced))
    with _LOCK:
        st = _COVER.setdefault(device, {"on": False, "pending": False})
        if st["pending"]:          # the last plane was never read: stop recording
            st["on"] = False
        st["pending"] = on = st["on"]
    return _lib.with_cover(tune, on)


def _cover_taken(device, tune):
    """A texture render took a silhouette render's workspace over: -> the ws_ready value for the C ABI."""
    with _LOCK:
        st = _COVER.setdefault(device, {"on": False, "pending": False})
        st["on"], st["pending"] = True, False
    return 2 if (tune is not None and tune.flags & 4) else 1


@dataclasses.dataclass
class _Setup:
    """An entry of _SETUP."""
    key: tuple
    inputs: tuple          # (v, c, f): kept alive, so that their addresses in the key cannot be recycled
    ws: torch.Tensor
    nbytes: int
    blur: float
    tune: object
    prefill: tuple = None  # the texture-output buffers the silhouette render pre-filled: handed out once (_take_prefill)


def _remember_setup(v, c, f, H, offset_z, ws, nb, blur, tune, prefill=None):
    if _SHARE[0]:
        ent = _Setup(_setup_key(v, c, f, H, offset_z), (v, c, f), ws, nb, float(blur), tune, prefill)
        with _LOCK:
            _SETUP[v.device] = ent


def _take_prefill(ent, N, H):
    """The texture-output buffers (imgs, sil, pix_to_face, texel_idx) that the silhouette render of a shared setup
    pre-filled on the empty blocks -- handed out once -- or None."""
    with _LOCK:
        pf, ent.prefill = ent.prefill, None
    return pf if (pf is not None and tuple(pf[0].shape) == (N, 3, H, H)) else None


def _shared_setup(v, c, f, H, offset_z):
    """-> (ws, nbytes, blur, tuning, prefill holder: the _Setup) of a silhouette render of exactly these inputs, or
    None."""
    with _LOCK:
        ent = _SETUP.get(v.device) if _SHARE[0] else None
    if ent is not None and ent.key == _setup_key(v, c, f, H, offset_z):
        return ent.ws, ent.nbytes, ent.blur, ent.tune, ent
    return None


# ------------------------------------------------------------------------------ projection
class _Project(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts, cams, offset_z):
        _lib.require_gpu(verts, cams)
        v, c = _f32c(verts), _f32c(cams)
        N, V, _ = v.shape
        out = torch.empty_like(v)
        _lib.call("acfm_project", v.device, _lib.ptr(v), _lib.ptr(c), N, V, float(offset_z), _lib.ptr(out))
        ctx.save_for_backward(v, c)
        return out

    @staticmethod
    def backward(ctx, g):
        v, c = ctx.saved_tensors
        N, V, _ = v.shape
        g = _f32c(g)
        gv = torch.empty_like(v) if ctx.needs_input_grad[0] else None
        gc = torch.empty_like(c) if ctx.needs_input_grad[1] else None
        _lib.call("acfm_project_backward", v.device, _lib.ptr(v), _lib.ptr(c), _lib.ptr(g), N, V, _lib.ptr(gv),
                  _lib.ptr(gc))
        return gv, gc, None


class _ProjectXY(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts, cams, offset_z):
        _lib.require_gpu(verts, cams)
        v, c = _f32c(verts), _f32c(cams)
        N, V, _ = v.shape
        out = torch.empty((N, V, 2), dtype=torch.float32, device=v.device)
        _lib.call("acfm_project_xy", v.device, _lib.ptr(v), _lib.ptr(c), N, V, float(offset_z), _lib.ptr(out))
        ctx.save_for_backward(v, c)
        return out

    @staticmethod
    def backward(ctx, g):
        v, c = ctx.saved_tensors
        N, V, _ = v.shape
        g = _f32c(g)
        gv = torch.empty_like(v) if ctx.needs_input_grad[0] else None
        gc = torch.empty_like(c) if ctx.needs_input_grad[1] else None
        _lib.call("acfm_project_xy_backward", v.device, _lib.ptr(v), _lib.ptr(c), _lib.ptr(g), N, V, _lib.ptr(gv),
                  _lib.ptr(gc))
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
        _lib.call("acfm_deform_apply", m.device, _lib.ptr(m), _lib.ptr(p), _lib.ptr(d), N, V, Kh, _lib.ptr(out))
        ctx.save_for_backward(p, d)
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
        _lib.call("acfm_deform_apply_backward", g.device, _lib.ptr(p), _lib.ptr(d), _lib.ptr(g), N, V, Kh, _lib.ptr(gd),
                  _lib.ptr(gm), None)
        if gp is not None:
            # dL/dP = sum_n g_n delta_n^T feeds the solve's backward, which amplifies its rounding by the conditioning
            # of the system: summed in double and rounded once (acfm_deform_presolve_sums_f64), so that the value does
            # not depend on how the frames are grouped; a frame-sharded step (sharding.SharedShapeExchange) takes the
            # unrounded doubles for its exchange buffer
            sink = _PRESOLVE_SINKS.get(p.data_ptr())
            if sink is not None:       # (G [V,K_h], sum g [V,3]): float64 views INSIDE the exchange buffer
                g64, m64 = sink.presolve_buffer(V, Kh, g.device)
            else:
                g64, m64 = torch.empty((V, Kh), dtype=torch.float64, device=g.device), None
            _lib.call("acfm_deform_presolve_sums_f64", g.device, _lib.ptr(d), _lib.ptr(g), N, V, Kh, _lib.ptr(g64),
                      _lib.ptr(m64), _lib.ptr(gp))
        return gm, gp, gd


# P leaf (data_ptr) -> the object that wants the unrounded double sums of its backward (presolve_buffer(V, Kh, device)
# -> persistent float64 tensors ([V,K_h], [V,3]) it will read after the backward).  One entry per live exchange.
_PRESOLVE_SINKS = {}


def register_presolve_sink(P, sink, previous_key=None):
    """sharding.SharedShapeExchange.apply(): the backward of deform_apply(., P, .) writes sum_n g_n delta_n^T in double
    into sink.presolve_buffer(...).  -> the key to hand back as previous_key next time (or to drop_presolve_sink)."""
    with _LOCK:
        if previous_key is not None:
            _PRESOLVE_SINKS.pop(previous_key, None)
        key = P.data_ptr()
        _PRESOLVE_SINKS[key] = sink
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
        _lib.call("acfm_deform_solve", b.device, _lib.ptr(l), _lib.ptr(b), V, Kh, _lib.ptr(P), _lib.ptr(ws), nbytes)
        if check:
            info = ctypes.c_int(0)
            _lib.call("acfm_deform_solve_info", b.device, _lib.ptr(ws), nbytes, V, ctypes.byref(info))
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
        _lib.call("acfm_deform_solve_backward", g.device, _lib.ptr(g), V, Kh, _lib.ptr(ctx.ws), ctx.ws.numel(),
                  _lib.ptr(gl))
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
class _CameraPipeline(torch.autograd.Function):
    @staticmethod
    def forward(ctx, emb, mirror_flag, transforms, decay):
        _lib.require_gpu(emb, mirror_flag, transforms)
        e = _f32c(emb)
        R = e.numel() // 7
        mf = mirror_flag.detach().reshape(-1).to(torch.int64).contiguous()
        tr = _f32c(transforms).reshape(-1, 4)
        N = mf.numel()
        if tr.shape[0] != N or R % N != 0:
            raise ValueError("camera rows %d must be a multiple of the %d frames (transforms %s)"
                             % (R, N, tuple(tr.shape)))
        out = torch.empty((R, 7), dtype=torch.float32, device=e.device)
        _lib.call("acfm_camera_pipeline", e.device, _lib.ptr(e), _lib.ptr(mf), _lib.ptr(tr), R, N, float(decay),
                  _lib.ptr(out))
        ctx.save_for_backward(e, mf, tr)
        ctx.decay = float(decay)
        return out

    @staticmethod
    def backward(ctx, g):
        e, mf, tr = ctx.saved_tensors
        R, N = e.numel() // 7, mf.numel()
        g = _f32c(g)
        ge = torch.empty_like(e)
        _lib.call("acfm_camera_pipeline_backward", e.device, _lib.ptr(e), _lib.ptr(mf), _lib.ptr(tr), _lib.ptr(g), R, N,
                  ctx.decay, _lib.ptr(ge))
        return ge, None, None, None


def camera_pipeline(cam_emb, mirror_flag, transforms, scale_lr_decay=1.0):
    """Camera embeddings [G,N,7] (or [R,7], row r of frame r % N) -> cameras [R,7]: decode, mirror by
    the per-frame flag [N], crop/scale transform [N,4] (multiframe/main.py:551-584) in one kernel."""
    return _CameraPipeline.apply(cam_emb, mirror_flag, transforms, scale_lr_decay)


class _CameraPipelineTables(torch.autograd.Function):
    @staticmethod
    def forward(ctx, frames_idx, selected, mirror_flag, transforms, decay, G, *tables):
        _lib.require_gpu(frames_idx, mirror_flag, transforms, *tables)
        ts = [_f32c(t) for t in tables]
        F = ts[0].shape[0]
        if not 1 <= len(ts) <= 32 or any(t.dim() != 2 or tuple(t.shape) != (F, 7) for t in ts):
            raise ValueError("camera_pipeline_tables: 1..32 embedding tables [frames, 7] of one size")
        fi = frames_idx.detach().reshape(-1).to(torch.int64).contiguous()
        mf = mirror_flag.detach().reshape(-1).to(torch.int64).contiguous()
        tr = _f32c(transforms).reshape(-1, 4)
        N = fi.numel()
        R = int(G) * N
        sel = None if selected is None else selected.detach().reshape(-1).to(torch.int64).contiguous()
        if mf.numel() != N or tr.shape[0] != N or (sel is not None and sel.numel() != R) or \
                (sel is None and int(G) > len(ts)):
            raise ValueError("camera_pipeline_tables: %d frames, mirror flags %d, transforms %s, G = %d, %d tables"
                             % (N, mf.numel(), tuple(tr.shape), G, len(ts)))
        out = torch.empty((R, 7), dtype=torch.float32, device=ts[0].device)
        ptrs = (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        _lib.call("acfm_camera_pipeline_tables", out.device, ptrs, len(ts), F, _lib.ptr(fi), _lib.ptr(sel), _lib.ptr(mf),
                  _lib.ptr(tr), R, N, float(decay), _lib.ptr(out))
        ctx.save_for_backward(fi, mf, tr, *ts) if sel is None else ctx.save_for_backward(fi, mf, tr, sel, *ts)
        ctx.cfg = (float(decay), R, N, F, len(ts), sel is not None)
        return out

    @staticmethod
    def backward(ctx, g):
        decay, R, N, F, nt, has_sel = ctx.cfg
        saved = ctx.saved_tensors
        fi, mf, tr = saved[:3]
        sel = saved[3] if has_sel else None
        ts = saved[4:] if has_sel else saved[3:]
        g = _f32c(g)
        need = ctx.needs_input_grad[6:]
        outs = [torch.empty((F, 7), dtype=torch.float32, device=g.device) if need[i] else None for i in range(nt)]
        ptrs = (ctypes.c_void_p * nt)(*[t.data_ptr() for t in ts])
        gptrs = (ctypes.c_void_p * nt)(*[(o.data_ptr() if o is not None else None) for o in outs])
        _lib.call("acfm_camera_pipeline_tables_backward", g.device, ptrs, nt, F, _lib.ptr(fi), _lib.ptr(sel), _lib.ptr(mf),
                  _lib.ptr(tr), _lib.ptr(g), R, N, decay, gptrs)
        return (None,) * 6 + tuple(outs)


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
        nf = tables[0].shape[0]
        lo, hi = int(frames_idx.min()), int(frames_idx.max())
        if lo < 0 or hi >= nf:
            raise IndexError("camera_pipeline_tables: frames_idx in [%d, %d] outside the %d rows of the embedding tables"
                             % (lo, hi, nf))
        if selected is not None and (int(selected.min()) < 0 or int(selected.max()) >= len(tables)):
            raise IndexError("camera_pipeline_tables: selected hypothesis outside the %d tables" % len(tables))
    return _CameraPipelineTables.apply(frames_idx, selected, mirror_flag, transforms, scale_lr_decay, G, *tables)


def camera_mirror(cams):
    """Decoded cameras [R,7] -> the pose of the horizontally flipped image (multiframe/main.py:97-125 with the flag
    set), one kernel; no gradient (the texture render it feeds sends none to its cameras)."""
    _lib.require_gpu(cams)
    c = _f32c(cams.detach()).reshape(-1, 7)
    out = torch.empty_like(c)
    _lib.call("acfm_camera_mirror", c.device, _lib.ptr(c), c.shape[0], _lib.ptr(out))
    return out


class _CameraNormalize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, raw):
        _lib.require_gpu(raw)
        r = _f32c(raw)
        N = r.numel() // 7
        out = torch.empty_like(r)
        _lib.call("acfm_camera_normalize", r.device, _lib.ptr(r), N, _lib.ptr(out))
        ctx.save_for_backward(r)
        return out

    @staticmethod
    def backward(ctx, g):
        (r,) = ctx.saved_tensors
        g = _f32c(g)
        gr = torch.empty_like(r)
        _lib.call("acfm_camera_normalize_backward", r.device, _lib.ptr(r), _lib.ptr(g), r.numel() // 7, _lib.ptr(gr))
        return gr


def camera_normalize(cam_raw):
    """[N,7] (s, tx, ty, q) -> (s, tx, ty, q/|q|): torch.cat([scale, trans, F.normalize(quat)]) in one kernel."""
    return _CameraNormalize.apply(cam_raw)


# ------------------------------------------------------------------------------ optical flow
class _OFLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, proj, flows, vis, B, T, masks, flip_t):
        _lib.require_gpu(proj, flows, vis)
        p, fl = _f32c(proj), _f32c(flows)
        V = p.shape[-2]
        H, W = fl.shape[-3], fl.shape[-2]
        vi = vis.detach().reshape(-1, V).to(torch.uint8).contiguous()
        clips = fl.numel() // (T * H * W * 2)
        mk = None if masks is None else _f32c(masks)
        if p.numel() != B * T * V * 3 or clips < 1 or fl.numel() != clips * T * H * W * 2 or B % clips != 0 or \
                vi.shape[0] != B * T or (mk is not None and mk.numel() != clips * T * H * W):
            raise ValueError("of_loss: proj %s flows %s vis %s masks %s do not match B=%d T=%d"
                             % (tuple(p.shape), tuple(fl.shape), tuple(vi.shape),
                                None if mk is None else tuple(mk.shape), B, T))
        loss = torch.empty((B, T - 1), dtype=torch.float32, device=p.device)
        cnt = torch.empty((B, T - 1), dtype=torch.float32, device=p.device)
        _lib.call("acfm_of_loss_shared", p.device, _lib.ptr(p), _lib.ptr(fl), _lib.ptr(mk), _lib.ptr(vi), B, T, V, H, W,
                  clips, int(bool(flip_t)), _lib.ptr(loss), _lib.ptr(cnt))
        ctx.save_for_backward(p, fl, vi, cnt) if mk is None else ctx.save_for_backward(p, fl, vi, cnt, mk)
        ctx.dims = (B, T, V, H, W, clips, int(bool(flip_t)), mk is not None)
        return loss

    @staticmethod
    def backward(ctx, g):
        B, T, V, H, W, clips, flip_t, has_m = ctx.dims
        p, fl, vi, cnt = ctx.saved_tensors[:4]
        mk = ctx.saved_tensors[4] if has_m else None
        g = _f32c(g)
        gp = torch.empty_like(p)
        _lib.call("acfm_of_loss_shared_backward", p.device, _lib.ptr(p), _lib.ptr(fl), _lib.ptr(mk), _lib.ptr(vi),
                  _lib.ptr(cnt), _lib.ptr(g), B, T, V, H, W, clips, flip_t, _lib.ptr(gp))
        return gp, None, None, None, None, None, None


def of_loss(proj, flows, vis, B, T, masks=None, flip_t=False):
    """Optical-flow loss per clip and frame pair [B,T-1] from projected vertices [B*T,V,3], GT flow
    images and the visible-vertex bitmap [B*T,V] (loss_utils.py:445-474, one kernel).  flows: [B*T,H,W,2], or
    [clips*T,H,W,2] with B a multiple of clips (rendered clip c reads clip c % clips: the hypotheses of a clip share its
    data); flip_t: frame k reads frame T-1-k; masks [clips*T,H,W]: the flow is multiplied by the mask of frame k at the
    sampled pixel -- i.e. main.py:676-686's flip / mask / repeat(G) of the flow images without materialising them."""
    return _OFLoss.apply(proj, flows, vis, int(B), int(T), masks, bool(flip_t))


# ------------------------------------------------------------------------------ flow operators: the switch
# Process-wide and read at call time (flow_ops.set_trainable / flow_ops.trainable are its public face).  Deliberately not
# thread-local: nn.DataParallel's replica threads must see what the main thread set.
_FLOW_TRAINABLE = False

_FORWARD_ONLY = ("%s: forward only (frozen flow network); wrap the call in torch.no_grad(), or opt in to the backward "
                 "kernels with flow_ops.set_trainable(True) / `with flow_ops.trainable():`")


def _once(fn):
    return torch.autograd.function.once_differentiable(fn)


# ------------------------------------------------------------------------------ correlation
def _correlation_args(f1, f2, max_displacement):
    _lib.require_gpu(f1, f2)
    a, b = _f32c(f1), _f32c(f2)
    if a.dim() != 4 or a.shape != b.shape:
        raise ValueError("correlation: two [N,C,H,W] tensors of equal shape, got %s and %s" % (tuple(a.shape), tuple(b.shape)))
    return a, b, int(max_displacement)


def _correlation_forward(a, b, md):
    N, C, H, W = a.shape
    out = torch.empty((N, (2 * md + 1) ** 2, H, W), dtype=torch.float32, device=a.device)
    _lib.call("acfm_correlation_forward", a.device, _lib.ptr(a), _lib.ptr(b), N, C, H, W, md, _lib.ptr(out))
    return out


class _Correlation(torch.autograd.Function):
    """Saves f1 and f2 only; the backward computes the side(s) asked for, each with its own launch."""

    @staticmethod
    def forward(ctx, f1, f2, md):
        a, b, md = _correlation_args(f1, f2, md)
        ctx.save_for_backward(a, b)
        ctx.md, ctx.dtypes = md, (f1.dtype, f2.dtype)
        return _correlation_forward(a, b, md)

    @staticmethod
    @_once
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        N, C, H, W = a.shape
        go = _f32c(g)
        g1 = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        g2 = torch.empty_like(b) if ctx.needs_input_grad[1] else None
        _lib.call("acfm_correlation_backward", a.device, _lib.ptr(go), _lib.ptr(a), _lib.ptr(b), N, C, H, W, ctx.md,
                  _lib.ptr(g1), _lib.ptr(g2))
        return (None if g1 is None else g1.to(ctx.dtypes[0]), None if g2 is None else g2.to(ctx.dtypes[1]), None)


def correlation(f1, f2, max_displacement):
    """Cost volume of MaskFlownet's Correlation layer (pad = max_displacement = md, kernel 1, strides 1):
    f1, f2 [N,C,H,W] -> [N,(2md+1)^2,H,W].  Forward only (the flow network is frozen in ACFM) unless
    `flow_ops.trainable()` is on: then a call that needs gradients goes through the backward kernel
    (acfm_correlation_backward: both sides are fixed-order gathers, bit-reproducible), with the same forward bits."""
    if torch.is_grad_enabled() and (f1.requires_grad or f2.requires_grad):
        _lib.require_gpu(f1, f2)
        if not _FLOW_TRAINABLE:
            raise RuntimeError(_FORWARD_ONLY % "correlation")
        return _Correlation.apply(f1, f2, int(max_displacement))
    return _correlation_forward(*_correlation_args(f1, f2, max_displacement))


# ------------------------------------------------------------------------------ deformable convolution
def _dconv_args(input, offset, weight, bias, shared_offset):
    _lib.require_gpu(input, offset, weight, bias)
    x, o, w = _f32c(input), _f32c(offset), _f32c(weight)
    b = None if bias is None else _f32c(bias)
    if x.dim() != 4:
        raise ValueError("deform_conv2d: input must be [N,Cin,H,W], got %s" % (tuple(x.shape),))
    N, Cin, H, W = x.shape
    if w.dim() != 4 or w.shape[1] != Cin or tuple(w.shape[2:]) != (3, 3):
        raise ValueError("deform_conv2d: weight must be [Cout,%d,3,3], got %s" % (Cin, tuple(w.shape)))
    Cout = w.shape[0]
    och = 2 if shared_offset else 18
    if tuple(o.shape) != (N, och, H, W):
        raise ValueError("deform_conv2d: offset must be [%d,%d,%d,%d]%s, got %s"
                         % (N, och, H, W, " (shared_offset)" if shared_offset else "", tuple(o.shape)))
    if b is not None and tuple(b.shape) != (Cout,):
        raise ValueError("deform_conv2d: bias must be [%d], got %s" % (Cout, tuple(b.shape)))
    if min(N, Cin, H, W, Cout) < 1:
        raise ValueError("deform_conv2d: empty input %s or weight %s" % (tuple(x.shape), tuple(w.shape)))
    return x, o, w, b


def _dconv_forward(x, o, w, b, shared_offset):
    (N, Cin, H, W), Cout = x.shape, w.shape[0]
    out = torch.empty((N, Cout, H, W), dtype=torch.float32, device=x.device)
    _lib.call("acfm_deform_conv2d_forward", x.device, _lib.ptr(x), _lib.ptr(o), _lib.ptr(w), _lib.ptr(b), N, Cin, H, W,
              Cout, 1 if shared_offset else 0, _lib.ptr(out))
    return out


class _DeformConv2d(torch.autograd.Function):
    """Saves input, offset and weight only (no columns, no tap tables: the backward recomputes the sampling)."""

    @staticmethod
    def forward(ctx, input, offset, weight, bias, shared_offset):
        x, o, w, b = _dconv_args(input, offset, weight, bias, shared_offset)
        ctx.save_for_backward(x, o, w)
        ctx.shared = bool(shared_offset)
        ctx.dtypes = tuple(None if t is None else t.dtype for t in (input, offset, weight, bias))
        return _dconv_forward(x, o, w, b, shared_offset)

    @staticmethod
    @_once
    def backward(ctx, g):
        x, o, w = ctx.saved_tensors
        (N, Cin, H, W), Cout = x.shape, w.shape[0]
        need = ctx.needs_input_grad
        go = _f32c(g)                                      # (the stride-0 gradient of out.sum() becomes a real tensor)
        new = lambda t, on: torch.empty_like(t) if on else None
        gx, goff, gw = new(x, need[0]), new(o, need[1]), new(w, need[2])
        gb = torch.empty((Cout,), dtype=torch.float32, device=x.device) if need[3] else None
        ws, nbytes = None, 0
        if gw is not None:
            nbytes = int(_lib.lib().acfm_deform_conv2d_backward_workspace_bytes(N, Cin, H, W, Cout))
            ws = torch.empty((max(nbytes, 4) // 4,), dtype=torch.float32, device=x.device)
        _lib.call("acfm_deform_conv2d_backward", x.device, _lib.ptr(go), _lib.ptr(x), _lib.ptr(o), _lib.ptr(w), N, Cin, H,
                  W, Cout, 1 if ctx.shared else 0, _lib.ptr(gx), _lib.ptr(goff), _lib.ptr(gw), _lib.ptr(gb), _lib.ptr(ws),
                  nbytes)
        return tuple(None if t is None else t.to(dt) for t, dt in zip((gx, goff, gw, gb), ctx.dtypes)) + (None,)


def deform_conv2d(input, offset, weight, bias=None, shared_offset=False):
    """torchvision's deform_conv2d in MaskFlownet's configuration (3x3, stride 1, padding 1, dilation 1, one group,
    one offset group, no mask): input [N,Cin,H,W], offset [N,18,H,W] (channel 2t the row offset, 2t+1 the column
    offset of tap t = 3 ky + kx), weight [Cout,Cin,3,3], bias [Cout] or None -> [N,Cout,H,W].  shared_offset: offset
    is [N,2,H,W] and every tap reads it -- offset.repeat(1, 9, 1, 1), which is what MaskFlownet's unsqueeze(1) /
    repeat_interleave(.., 9, 1) / view builds, without the copy and with the same bits.  Forward only (the flow
    network is frozen in ACFM) unless `flow_ops.trainable()` is on: then a call that needs gradients goes through
    acfm_deform_conv2d_backward with the same forward bits (the shared form gets the gradient of the [N,2,H,W] offset
    itself; grad_input is added atomically and does not repeat its bits, the other gradients do; at an integer sample
    coordinate the offset gradient is the floor cell's, torchvision's convention)."""
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (input, offset, weight, bias)):
        _lib.require_gpu(input, offset, weight, bias)
        if not _FLOW_TRAINABLE:
            raise RuntimeError(_FORWARD_ONLY % "deform_conv2d")
        return _DeformConv2d.apply(input, offset, weight, bias, bool(shared_offset))
    return _dconv_forward(*_dconv_args(input, offset, weight, bias, shared_offset), shared_offset)


# ------------------------------------------------------------------------------ lazy pix_to_face
class LazyPixToFace(torch.Tensor):
    """`pix_to_face [N,H,W,K]` int64 as the reference's renderer returns it, with the K-1 planes nobody in the training
    path reads produced on first use.  The render writes the nearest-face plane (all that loss_utils.py:214 `[..., 0]`
    and :431 `[..., :1]` read: 8 bytes per pixel instead of 8 K); `p[..., 0]` and `p[..., :1]` are views of it; splitting
    along the batch dimension (`p[a:b]`, `p[n]`, `chunk` / `split` on dim 0 -- what nn.DataParallel's scatter does to
    every tensor argument, main.py:326, 718, also on one device) gives lazy tensors over the parts; ANY other
    operation (indexing another slot, .cpu(), comparisons, printing ...) first renders the full tensor -- the same
    kernel once more with all K slots stored, from the very tensors of the original call -- and then behaves like the
    plain tensor.  If those inputs changed meanwhile (in-place write, invalidate_setups()) it raises instead of
    returning ids of other geometry: NeuralRenderer(pix_to_face_slots=K) stores all K slots at render time."""

    @staticmethod
    def __new__(cls, plane0, K, make_full, vis=None):
        shape = tuple(plane0.shape[:-1]) + (int(K),)
        r = torch.Tensor._make_wrapper_subclass(cls, shape, dtype=plane0.dtype, device=plane0.device)
        r._plane0, r._make_full, r._full = plane0, make_full, None
        r._acfm_vis = vis
        return r

    @property
    def is_materialized(self):
        return self._full is not None

    def materialize(self):
        if self._full is None:
            self._full = self._make_full()
            self._make_full = None
        return self._full

    def __repr__(self):
        return "LazyPixToFace(shape=%s, materialized=%s)" % (tuple(self.shape), self.is_materialized)

    def __deepcopy__(self, memo):
        return self.materialize().clone()

    def _rows(self, start, end, squeeze=False):
        """Lazy tensor over meshes start..end-1 (squeeze: the single mesh `start`, batch dimension dropped)."""
        parent = self
        pl = self._plane0[start] if squeeze else self._plane0[start:end]
        vis = self._acfm_vis
        if vis is not None:
            vis = None if squeeze else vis[start:end]
        return LazyPixToFace(pl, self.shape[-1], (lambda: parent.materialize()[start] if squeeze
                                                  else parent.materialize()[start:end]), vis)

    @classmethod
    def __torch_dispatch__(cls, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        a0 = args[0] if args else None
        if isinstance(a0, LazyPixToFace) and a0._full is None:
            nd = a0.dim()
            aten = torch.ops.aten
            dim = args[1] if len(args) > 1 and isinstance(args[1], int) else None
            last = dim in (nd - 1, -1) and nd > 1
            first = dim in (0, -nd) and nd == 4
            if func is aten.select.int and last and args[2] == 0:
                return a0._plane0.select(nd - 1, 0)
            if func is aten.slice.Tensor and last and len(args) >= 4 and args[2] in (0, None) and args[3] == 1 and \
                    (len(args) < 5 or args[4] == 1):
                return a0._plane0
            if func in (aten.detach.default, aten.alias.default):
                return a0
            N = a0.shape[0]
            if func is aten.select.int and first:
                i = args[2] + N if args[2] < 0 else args[2]
                if 0 <= i < N:
                    return a0._rows(i, i + 1, squeeze=True)
            if func is aten.slice.Tensor and (first or (len(args) == 1 and nd == 4)) and (len(args) < 5 or args[4] == 1):
                lo = args[2] if len(args) > 2 and args[2] is not None else 0
                hi = args[3] if len(args) > 3 and args[3] is not None else N
                lo = max(0, lo + N if lo < 0 else lo)
                hi = min(N, hi + N if hi < 0 else hi)
                if lo < hi:
                    return a0._rows(lo, hi)
            if func is aten.split.Tensor and (len(args) < 3 or args[2] in (0, -nd)) and nd == 4 and args[1] > 0:
                return [a0._rows(lo, min(N, lo + args[1])) for lo in range(0, N, args[1])]
            if func is aten.split_with_sizes.default and (len(args) < 3 or args[2] in (0, -nd)) and nd == 4 and \
                    sum(args[1]) == N and all(x > 0 for x in args[1]):
                out, lo = [], 0
                for x in args[1]:
                    out.append(a0._rows(lo, lo + x))
                    lo += x
                return out
        from torch.utils._pytree import tree_map
        unwrap = lambda x: x.materialize() if isinstance(x, LazyPixToFace) else x
        return func(*tree_map(unwrap, args), **tree_map(unwrap, kwargs))


def _lazy_pix_to_face(plane0, vis, v, f, c, H, K, blur, sigma, offset_z):
    """Wraps the nearest-face plane of a silhouette render (see LazyPixToFace)."""
    versions = (v._version, f._version, c._version, _EPOCH[0])
    tune = _lib.tuning()[1]
    born_in = _capture_id(v.device)

    def make_full():
        if (v._version, f._version, c._version, _EPOCH[0]) != versions:
            raise RuntimeError("pix_to_face: slots beyond [..., 0] are rendered on first use, but the vertices / faces / "
                               "cameras of that render have been modified since (in-place write, or a hipGraph replay "
                               "announced with invalidate_setups()); "
                               "use NeuralRenderer(pix_to_face_slots=faces_per_pixel) to store every slot at render time")
        if _capture_id(v.device) != born_in:
            # made while a hipGraph was being captured: its inputs are the capture's buffers, which hold nothing until a
            # replay and whatever the last replay left afterwards -- there is no "the render's inputs" to re-render from
            raise RuntimeError("pix_to_face: this tensor was rendered inside a hipGraph capture; its slots beyond [..., 0] "
                               "can only be formed inside that same capture.  Use NeuralRenderer(pix_to_face_slots="
                               "faces_per_pixel) in captured steps that read them")
        N, V, _ = v.shape
        F = f.shape[1]
        mask = torch.empty((N, H, H), dtype=torch.float32, device=v.device)
        full = torch.empty((N, H, H, K), dtype=torch.int64, device=v.device)
        kth = torch.empty((N, H, H), dtype=torch.int64, device=v.device)
        vis2 = torch.empty((N, V), dtype=torch.uint8, device=v.device)
        ws, nb = _workspace(N, V, F, H, v.device)          # its own workspace: the render's is still the backward's
        _lib.call("acfm_sil_forward", v.device, _lib.ptr(v), _lib.ptr(f), _lib.ptr(c), N, V, F, H, K, K, float(blur),
                  float(sigma), float(offset_z), _lib.ptr(mask), _lib.ptr(full), _lib.ptr(kth), _lib.ptr(vis2),
                  _lib.ptr(ws), nb, _lib.tuning_ptr(tune))
        return full

    return LazyPixToFace(plane0, K, make_full, vis)


# The reference computes its losses on the rendered images with separate operators (main.py:644-662, 716-717), so the
# gradient of a loss with respect to a whole image -- [N,H,W] for the silhouette terms, [N,3,H,W] for the texture
# MSE -- is written by one kernel only to be read once by the render's backward.  Both backward kernels can form that
# gradient per pixel themselves (acfm_sil_loss_backward, acfm_tex_mse_backward_faces: the opt-in fused operators).
# LazyGrad lets the drop-in operators use them too: the loss operator's backward hands autograd a tensor of the right
# shape that merely REMEMBERS how the gradient is defined (the operator's inputs and its upstream gradient); the render's
# backward recognises it -- same image, untouched -- and calls the fused kernel.  Two things autograd does to such a
# gradient on the reference's own call sequence stay lazy: shape-only views (l1_loss / iou hand the operator
# `mask.view(N, -1)` / `mask[:, None]`, loss_utils.py:18-32, 72-77: the view's backward reshapes the gradient) and the
# SUM of the gradients of two silhouette-loss operators on the same mask (l1_loss and edt_loss, main.py:644 and :716:
# the sum is the gradient of one operator with both references and the two upstream gradients added).  ANY other use
# (a hook, another consumer's gradient added, torch.autograd.grad with respect to the image itself) forms the gradient
# with the loss operator's own backward kernel first and then behaves like the plain tensor.
LAZY_GRADS = [True]


def _same_tensor(a, b):
    return a is b or (a is not None and b is not None and a.data_ptr() == b.data_ptr() and a.shape == b.shape
                      and a._version == b._version and a.dtype == b.dtype)


class LazyGrad(torch.Tensor):
    @staticmethod
    def __new__(cls, like, tag, payload, make_full, shape=None):
        r = torch.Tensor._make_wrapper_subclass(cls, tuple(like.shape) if shape is None else tuple(shape),
                                                dtype=like.dtype, device=like.device)
        r._tag, r._payload, r._make_full, r._full = tag, payload, make_full, None
        return r

    @property
    def is_materialized(self):
        return self._full is not None

    def materialize(self):
        if self._full is None:
            self._full = self._make_full().reshape(self.shape)
            self._make_full = self._payload = None
        return self._full

    def take(self, tag, image):
        """The operator inputs behind this gradient if it is still unformed, of kind `tag`, and a gradient with
        respect to exactly `image` (same storage, element count and version); else None."""
        if self._full is not None or self._tag != tag:
            return None
        img = self._payload[0]
        if img.data_ptr() != image.data_ptr() or img.numel() != image.numel() or self.numel() != image.numel() or \
                img._version != image._version:
            return None
        return self._payload

    def _reshaped(self, shape):
        parent = self
        return LazyGrad(self, self._tag, self._payload, lambda: parent.materialize(), shape=shape)

    def _merged(self, other):
        """self + other for two unformed silhouette-loss gradients of the same mask, itself unformed; else None."""
        if self._full is not None or other._full is not None or self._tag != "mask_losses" or other._tag != "mask_losses" \
                or self.shape != other.shape:
            return None
        m1, g1, e1, rb1, go1 = self._payload
        m2, g2, e2, rb2, go2 = other._payload
        if not _same_tensor(m1, m2):
            return None
        if (g1 is not None and g2 is not None and not _same_tensor(g1, g2)) or \
                (e1 is not None and e2 is not None and not _same_tensor(e1, e2)):
            return None
        refs = [r for r in (g1, g2, e1, e2) if r is not None]
        if any(r.shape[0] != refs[0].shape[0] for r in refs):
            return None
        # a term whose reference an operator did not have contributes nothing to that operator's gradient
        # (acfm_mask_losses_backward skips it): mask its columns before the two upstream gradients are added
        def cols(go, g, e):
            if g is not None and e is not None:
                return go
            return go * _lib.const((1.0, 1.0, 1.0, 0.0) if e is None else (0.0, 0.0, 0.0, 1.0), go.device)
        go = cols(go1, g1, e1) + cols(go2, g2, e2)
        g, e = (g1 if g1 is not None else g2), (e1 if e1 is not None else e2)
        rb = refs[0].shape[0] if refs else m1.shape[0]
        a, b = self, other

        def make():
            return a.materialize() + b.materialize()
        return LazyGrad(self, "mask_losses", (m1, g, e, rb, go), make)

    def __repr__(self):
        return "LazyGrad(%s, shape=%s, materialized=%s)" % (self._tag, tuple(self.shape), self.is_materialized)

    @classmethod
    def __torch_dispatch__(cls, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        aten = torch.ops.aten
        a0 = args[0] if args else None
        if type(a0) is LazyGrad and a0._full is None:
            if func in (aten.detach.default, aten.alias.default):
                return a0
            if func in (aten.view.default, aten.reshape.default, aten._unsafe_view.default):
                shape = list(args[1])
                if -1 in shape:
                    known = 1
                    for x in shape:
                        known *= x if x != -1 else 1
                    shape[shape.index(-1)] = a0.numel() // max(known, 1)
                n = 1
                for x in shape:
                    n *= x
                if n == a0.numel():
                    return a0._reshaped(shape)
            if func is aten.squeeze.dim and a0.shape[args[1]] == 1:
                shape = list(a0.shape)
                del shape[args[1]]
                return a0._reshaped(shape)
            if func is aten.unsqueeze.default:
                shape = list(a0.shape)
                shape.insert(args[1] if args[1] >= 0 else args[1] + a0.dim() + 1, 1)
                return a0._reshaped(shape)
            if func is aten.add.Tensor and len(args) == 2 and type(args[1]) is LazyGrad and \
                    kwargs.get("alpha", 1) == 1:
                m = a0._merged(args[1])
                if m is not None:
                    return m
        from torch.utils._pytree import tree_map
        unwrap = lambda x: x.materialize() if type(x) is LazyGrad else x
        return func(*tree_map(unwrap, args), **tree_map(unwrap, kwargs))


# ------------------------------------------------------------------------------ silhouette
class _SilRender(torch.autograd.Function):
    """Soft silhouette render (acfm_sil_forward_ex / acfm_sil_backward_ex); fused=True: the render and its [N,4]
    silhouette-loss vector against gt / edt as one operator (acfm_sil_loss_forward_ex / acfm_sil_loss_backward_ex),
    the mask then carries no gradient.  -> (losses or None, mask, pix_to_face, vis, proj)."""

    @staticmethod
    def forward(ctx, verts, faces, cams, gt, edt, img_size, K, blur, sigma, offset_z, k_out, f16, fused):
        _lib.require_gpu(verts, faces, cams, gt, edt)
        v, c = _f32c(verts), _f32c(cams)
        N, V, _ = v.shape
        f = expand_faces(faces, N)
        F, H = f.shape[1], int(img_size)
        if f16 and k_out != 1:
            raise ValueError("storage='f16' writes the int32 nearest-face plane only (k_out = 1)")
        g = _real(gt, f16).reshape(-1, H, H) if gt is not None else None
        e = _real(edt, f16).reshape(-1, H, H) if edt is not None else None
        RB = N
        for r in (g, e):
            if r is not None:
                RB = _ref_batch(N, r, "sil_render_losses")
        if g is not None and e is not None and g.shape[0] != e.shape[0]:
            raise ValueError("sil_render_losses: gt and edt must have the same batch")
        mask = torch.empty((N, H, H), dtype=torch.float16 if f16 else torch.float32, device=v.device)
        p2f = torch.empty((N, H, H, k_out), dtype=torch.int32 if f16 else torch.int64, device=v.device)
        kth = torch.empty((N, H, H), dtype=torch.int64, device=v.device)  # u64 keys, opaque
        vis = torch.empty((N, V), dtype=torch.uint8, device=v.device)
        losses = torch.empty((N, 4), dtype=torch.float32, device=v.device) if fused else None
        ws, nb = _workspace(N, V, F, H, v.device)
        tune = _cover_tuning(v.device, _lib.tuning()[1])
        if f16:
            tune = _lib.with_f16(tune, True)
        tp = _lib.tuning_ptr(tune)
        # a texture render of this prediction is expected (the cover flag is on while they do follow): its constant
        # outputs on the empty blocks are stored by THIS kernel, behind the walk, into buffers that render then adopts
        # (acfm_sil_forward_prefill / acfm_tex_forward ws_ready = 3: -20 us of the texture kernel's 36)
        prefill = None
        if not fused and PREFILL_TEX[0] and tune is not None and (tune.flags & 4) and not f16 and _SHARE[0]:
            prefill = (torch.empty((N, 3, H, H), dtype=torch.float32, device=v.device),
                       torch.empty((N, H, H), dtype=torch.float32, device=v.device),
                       torch.empty((N, H, H, 1), dtype=torch.int64, device=v.device),
                       torch.empty((N, H, H), dtype=torch.int32, device=v.device))
        # NeuralRenderer.project_points of these very vertices and cameras (main.py:715, predictor.py:319: the boundary
        # loss's input) comes out of the face setup (AcfmSilExtras.proj_xy) and its gradient goes back through THIS
        # operator's one projection backward: no second projection kernel either way, no sum of two vertex / camera
        # gradients afterwards (k_project, k_project_bwd and two torch adds less per step)
        proj = torch.empty((N, V, 2), dtype=torch.float32, device=v.device)
        exp, _ex_keep = _lib.sil_extras(proj_xy=proj, prefill=prefill)
        P = _lib.ptr
        if fused:
            _lib.call("acfm_sil_loss_forward_ex", v.device, P(v), P(f), P(c), P(g), P(e), RB, N, V, F, H, K, int(k_out),
                      float(blur), float(sigma), float(offset_z), P(mask), P(p2f), P(kth), P(vis), P(losses), P(ws), nb,
                      tp, exp)
        else:
            _lib.call("acfm_sil_forward_ex", v.device, P(v), P(f), P(c), N, V, F, H, K, int(k_out), float(blur),
                      float(sigma), float(offset_z), P(mask), P(p2f), P(kth), P(vis), P(ws), nb, tp, exp)
        _remember_setup(v, c, f, H, offset_z, ws, nb, blur, tune, prefill)
        ctx.save_for_backward(v, f, c, mask, kth, g, e)
        ctx.cfg = (H, float(blur), float(sigma), float(offset_z), RB)
        ctx.ws = (ws, nb, tune)  # face records + tile schedule: reused by backward (no second setup)
        ctx.mark_non_differentiable(*((mask, p2f, vis) if fused else (p2f, vis)))
        ctx.set_materialize_grads(False)  # no zero-filled [N,H,H,K] int64 "gradient" for pix_to_face
        return losses, mask, p2f, vis, proj

    @staticmethod
    def backward(ctx, glosses, gmask, _gp2f, _gvis, gproj):
        v, f, c, mask, kth, g, e = ctx.saved_tensors
        H, blur, sigma, offset_z, RB = ctx.cfg
        N, V, _ = v.shape
        F = f.shape[1]
        none = (None,) * 13
        if glosses is None and gmask is None and gproj is None:
            return none
        gv = torch.empty_like(v) if ctx.needs_input_grad[0] else None
        gc = torch.empty_like(c) if ctx.needs_input_grad[2] else None
        gp = _f32c(gproj) if gproj is not None else None
        P = _lib.ptr
        if glosses is None and gmask is None:      # only the projection was used: its own backward
            _lib.call("acfm_project_xy_backward", v.device, P(v), P(c), P(gp), N, V, P(gv), P(gc))
            return (gv, None, gc) + none[3:]
        ws, nb, tune = ctx.ws
        exp, _ex_keep = _lib.sil_extras(grad_proj_xy=gp)
        if glosses is not None:       # the fused operator
            pay = (mask, g, e, RB, _f32c(glosses))
        else:                         # the silhouette losses' gradient, still unformed: the kernel forms it per pixel
            pay = gmask.take("mask_losses", mask) if type(gmask) is LazyGrad else None
        if pay is not None:
            _m, lg, le, rb, go = pay
            _lib.call("acfm_sil_loss_backward_ex", v.device, P(v), P(f), P(c), P(mask), P(kth), P(lg), P(le), rb, P(go),
                      N, V, F, H, blur, sigma, offset_z, P(gv), P(gc), P(ws), nb, 1, _lib.tuning_ptr(tune), exp)
        else:
            gm = _f32c(gmask)
            _lib.call("acfm_sil_backward_ex", v.device, P(v), P(f), P(c), P(mask), P(kth), P(gm), N, V, F, H, blur,
                      sigma, offset_z, P(gv), P(gc), P(ws), nb, 1, _lib.tuning_ptr(tune), exp)
        return (gv, None, gc) + none[3:]


def _proj_key(verts, cams):
    return (verts.data_ptr(), verts._version, tuple(verts.shape), str(verts.dtype), cams.data_ptr(), cams._version,
            tuple(cams.shape), str(cams.dtype))


def _sil_apply(verts, faces, cams, gt, edt, img_size, K, blur, sigma, offset_z, k_out, storage, fused):
    """_SilRender with the k_out / lazy resolution of both wrappers; -> (losses or None, mask, pix_to_face)."""
    f16 = _is_f16(storage)
    lazy = k_out == "lazy" and not f16 and K > 1
    losses, mask, p2f, vis, proj = _SilRender.apply(verts, faces, cams, gt, edt, img_size, K, blur, sigma, offset_z,
                                                    1 if (f16 or lazy) else (K if k_out in (None, "lazy") else int(k_out)),
                                                    f16, fused)
    if lazy:   # k_out="lazy": [N,H,H,K] whose slots 1.. are rendered on first use (LazyPixToFace)
        p2f = _lazy_pix_to_face(p2f, vis, _f32c(verts), expand_faces(faces, verts.shape[0]), _f32c(cams),
                                int(img_size), int(K), blur, sigma, offset_z)
    else:
        p2f._acfm_vis = vis
    # the (x, y) projection of these vertices under these cameras, an output of the render's autograd node: rides on
    # the pix_to_face object like the visibility bitmap (NeuralRenderer.project_points picks it up)
    p2f._acfm_proj = (_proj_key(verts, cams), proj)
    return losses, mask, p2f


def sil_render(verts, faces, cams, img_size, K=SIL_K, blur=SIL_BLUR, sigma=SIL_SIGMA, offset_z=0.0,
               k_out=None, storage="f32"):
    """Soft silhouette: -> (mask [N,H,H] f32, pix_to_face [N,H,H,k_out] i64), k_out = K (default,
    what PyTorch3D returns) or 1 (nearest-face plane only; K faces are still blended).
    The visible-vertex bitmap the raster kernel produces on the side (vertices of every
    nearest face, = what bds_loss / optical_flow_loss derive from pix_to_face[..., 0]) rides
    along on the pix_to_face tensor object as `._acfm_vis`.
    storage="f16": mask [N,H,H] float16, pix_to_face [N,H,H,1] int32 (BASELINE config 5); fp32 arithmetic."""
    return _sil_apply(verts, faces, cams, None, None, img_size, K, blur, sigma, offset_z, k_out, storage, False)[1:]


def sil_render_losses(verts, faces, cams, img_size, gt=None, edt=None, K=SIL_K, blur=SIL_BLUR, sigma=SIL_SIGMA,
                      offset_z=0.0, k_out=None, storage="f32"):
    """Soft-silhouette render and its silhouette losses as ONE operator (opt-in; the drop-in pair is
    sil_render + mask_losses): -> (losses [N,4] = (mean|m-gt|, sum m*gt, sum(m+gt-m*gt), mean edt*m), mask [N,H,H],
    pix_to_face [N,H,H,k_out]).  Gradients flow from `losses` to verts / cams; `mask` is returned for inspection and
    carries none (use sil_render when the mask itself feeds further differentiable code).  gt / edt: [N,...] or
    [N/G,...] shared by the G hypotheses of a frame.  storage="f16": the mask and the references are held in float16,
    the loss sums stay float32."""
    return _sil_apply(verts, faces, cams, gt, edt, img_size, K, blur, sigma, offset_z, k_out, storage, True)


# ------------------------------------------------------------------------------ hard raster
def hard_raster(verts_proj, faces, img_size):
    """OF_NeuralRenderer.forward: pre-projected verts -> pix_to_face [N,H,H,1] i64."""
    _lib.require_gpu(verts_proj, faces)
    v = _f32c(verts_proj)
    N, V, _ = v.shape
    f = expand_faces(faces, N)
    F, H = f.shape[1], int(img_size)
    p2f = torch.empty((N, H, H, 1), dtype=torch.int64, device=v.device)
    vis = torch.empty((N, V), dtype=torch.uint8, device=v.device)
    ws, nb = _workspace(N, V, F, H, v.device)
    _lib.call("acfm_hard_raster", v.device, _lib.ptr(v), _lib.ptr(f), N, V, F, H, _lib.ptr(p2f), _lib.ptr(vis),
              _lib.ptr(ws), nb, _lib.tuning()[0])
    p2f._acfm_vis = vis
    return p2f


# ------------------------------------------------------------------------------ rasterizer fragments
FRAGMENT_K = (1, 2, 4, 8, 10, 20, 32)


class _Fragments(torch.autograd.Function):
    """PyTorch3D rasterize_meshes over NDC / view-space vertices (acfm_rasterize_fragments /
    acfm_rasterize_fragments_backward) -> (pix_to_face, zbuf, bary_coords, dists); gradients to verts_ndc only."""

    @staticmethod
    def forward(ctx, verts_ndc, faces, H, K, blur, clip):
        _lib.require_gpu(verts_ndc, faces)
        v = _f32c(verts_ndc)
        N, V, _ = v.shape
        f = expand_faces(faces, N)
        F = f.shape[1]
        dev = v.device
        p2f = torch.empty((N, H, H, K), dtype=torch.int64, device=dev)
        zbuf = torch.empty((N, H, H, K), dtype=torch.float32, device=dev)
        bary = torch.empty((N, H, H, K, 3), dtype=torch.float32, device=dev)
        dists = torch.empty((N, H, H, K), dtype=torch.float32, device=dev)
        nb = _lib.lib().acfm_rasterize_fragments_workspace_bytes(N, V, F, H)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        tune = _lib.tuning()[1]
        P = _lib.ptr
        _lib.call("acfm_rasterize_fragments", dev, P(v), P(f), N, V, F, H, K, float(blur), int(clip), P(p2f), P(zbuf),
                  P(bary), P(dists), P(ws), nb, _lib.tuning_ptr(tune))
        ctx.save_for_backward(v, f, p2f)
        ctx.cfg = (H, K, float(blur), int(clip))
        ctx.ws = (ws, nb, tune)   # face records of the forward: the backward sets nothing up again
        ctx.mark_non_differentiable(p2f)
        ctx.set_materialize_grads(False)   # an unused output sends no gradient: that path is skipped, nothing read
        return p2f, zbuf, bary, dists

    @staticmethod
    def backward(ctx, _gp2f, gzbuf, gbary, gdists):
        none = (None,) * 5
        if not ctx.needs_input_grad[0] or (gzbuf is None and gbary is None and gdists is None):
            return (None,) + none
        v, f, p2f = ctx.saved_tensors
        H, K, blur, clip = ctx.cfg
        ws, nb, tune = ctx.ws
        N, V, _ = v.shape
        gz, gb, gd = (_f32c(g) if g is not None else None for g in (gzbuf, gbary, gdists))
        gv = torch.empty_like(v)
        P = _lib.ptr
        _lib.call("acfm_rasterize_fragments_backward", v.device, P(v), P(f), P(p2f), P(gz), P(gb), P(gd), N, V,
                  f.shape[1], H, K, blur, clip, P(gv), P(ws), nb, 1, _lib.tuning_ptr(tune))
        return (gv,) + none


def rasterize_fragments(verts_ndc, faces, image_size, faces_per_pixel, blur_radius=0.0, clip_barycentric_coords=False):
    """PyTorch3D 0.3.0 rasterize_meshes (naive path) of verts_ndc [N,V,3] = (NDC x, NDC y, view z), faces [F,3] or
    [N,F,3] -> (pix_to_face [N,H,H,K] i64 packed n*F+f, zbuf [N,H,H,K], bary_coords [N,H,H,K,3], dists [N,H,H,K]),
    -1 in every empty slot.  zbuf / bary_coords / dists are differentiable with respect to verts_ndc (any subset of
    them may be used).  K = faces_per_pixel in FRAGMENT_K; raster_tuning(deterministic=True) makes the backward
    bit-reproducible."""
    H, K = int(image_size), int(faces_per_pixel)
    if K not in FRAGMENT_K:
        raise ValueError("faces_per_pixel=%d is not supported (one of %s)" % (K, FRAGMENT_K))
    if not blur_radius >= 0.0:
        raise ValueError("blur_radius must be >= 0, got %r" % (blur_radius,))
    if verts_ndc.dim() != 3 or verts_ndc.shape[-1] != 3:
        raise ValueError("verts_ndc must be [N,V,3], got %s" % (tuple(verts_ndc.shape),))
    _lib.require_gpu(verts_ndc, faces)
    return _Fragments.apply(verts_ndc, faces, H, K, float(blur_radius), bool(clip_barycentric_coords))


# ------------------------------------------------------------------------------ shaders over fragments
# PyTorch3D 0.3.0's blends and interpolate_face_attributes over Fragments: flattened to
# P = N*H*W pixels of K slots, each a call of acfm_shade.hip.  Gradients to zbuf / bary_coords / dists go back into the
# fragments, and _Fragments.backward carries them to the vertices.
def _shade_storage(storage):
    if storage != "f32":
        raise ValueError("storage=%r: half storage is not supported on the shader path (float32 only)" % (storage,))


def _frag_planes(fragments):
    """Fragments (or a (pix_to_face, zbuf, bary_coords, dists) tuple) -> the four planes.  The kernels index every
    plane by pix_to_face's [N,H,W,K] layout, so the shapes are checked here: dists / zbuf [N,H,W,K], bary_coords
    [N,H,W,K,3], K in FRAGMENT_K.  (The device is checked by the caller, after its own shape checks.)"""
    p2f, zbuf, bary, dists = (fragments.pix_to_face, fragments.zbuf, fragments.bary_coords, fragments.dists) \
        if hasattr(fragments, "pix_to_face") else tuple(fragments)
    if p2f.dim() != 4:
        raise ValueError("pix_to_face must be [N,H,W,K], got %s" % (tuple(p2f.shape),))
    K = int(p2f.shape[-1])
    if K not in FRAGMENT_K:
        raise ValueError("faces_per_pixel=%d is not supported (one of %s)" % (K, FRAGMENT_K))
    shape = tuple(p2f.shape)
    for name, t, want in (("zbuf", zbuf, shape), ("dists", dists, shape), ("bary_coords", bary, shape + (3,))):
        if t is None or tuple(t.shape) != want:
            raise ValueError("fragments.%s must be %s like pix_to_face, got %s"
                             % (name, want, None if t is None else tuple(t.shape)))
    return p2f, zbuf, bary, dists


def _i64c(t):
    return t.detach().to(torch.int64).contiguous()


def _a16(t):
    """float32 contiguous, 16-byte aligned (the RGBA planes are read as float4)."""
    t = _f32c(t)
    return t if t.data_ptr() % 16 == 0 else t.clone()


def blend_struct(blend_params, znear=1.0, zfar=100.0):
    """BlendParams (sigma, gamma, background_color: a scalar or an RGB triple) -> the AcfmBlendParams structure."""
    bg = blend_params.background_color
    if torch.is_tensor(bg):
        bg = bg.detach().cpu().reshape(-1).tolist()
    bg = [float(bg)] * 3 if not isinstance(bg, (tuple, list)) else [float(c) for c in bg]
    if len(bg) == 1:
        bg = bg * 3
    if len(bg) != 3:
        raise ValueError("background_color must be a scalar or an RGB triple, got %r" % (blend_params.background_color,))
    if not (blend_params.sigma > 0 and blend_params.gamma > 0):
        raise ValueError("sigma and gamma must be > 0")
    return _lib.BlendParams(float(blend_params.sigma), float(blend_params.gamma), (ctypes.c_float * 3)(*bg),
                            float(znear), float(zfar))


def _det_ws(tune, n, dev):
    """Workspace of a scattering backward: 16 bytes per gradient element in deterministic mode, else none."""
    if tune is not None and tune.flags & 1:
        nb = 16 * n
        return torch.empty(nb, dtype=torch.uint8, device=dev), nb
    return None, 0


class _SigmoidBlend(torch.autograd.Function):
    """sigmoid_alpha_blend (acfm_sigmoid_alpha_blend{,_backward}) -> RGBA [N,H,W,4]; gradients to colors and dists."""

    @staticmethod
    def forward(ctx, colors, dists, p2f, sigma):
        p2f, d = _i64c(p2f), _f32c(dists)
        K = p2f.shape[-1]
        P = p2f.numel() // K
        c = _f32c(colors) if colors is not None else None
        rgba = torch.empty(p2f.shape[:-1] + (4,), dtype=torch.float32, device=p2f.device)
        tune = _lib.tuning()[1]
        _lib.call("acfm_sigmoid_alpha_blend", p2f.device, _lib.ptr(p2f), _lib.ptr(d), _lib.ptr(c), P, K, float(sigma),
                  _lib.ptr(rgba), _lib.tuning_ptr(tune))
        ctx.save_for_backward(p2f, d)
        ctx.cfg = (P, K, float(sigma), tune)
        ctx.set_materialize_grads(False)
        return rgba

    @staticmethod
    def backward(ctx, g):
        need_c, need_d = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if g is None or not (need_c or need_d):
            return None, None, None, None
        p2f, d = ctx.saved_tensors
        P, K, sigma, tune = ctx.cfg
        gd = torch.empty_like(d) if need_d else None
        gc = torch.empty(p2f.shape + (3,), dtype=torch.float32, device=p2f.device) if need_c else None
        _lib.call("acfm_sigmoid_alpha_blend_backward", p2f.device, _lib.ptr(p2f), _lib.ptr(d), _lib.ptr(_a16(g)), P, K,
                  sigma, _lib.ptr(gd), _lib.ptr(gc), _lib.tuning_ptr(tune))
        return gc, gd, None, None


class _SoftmaxBlend(torch.autograd.Function):
    """softmax_rgb_blend (acfm_softmax_rgb_blend{,_backward}) -> RGBA [N,H,W,4].  Colours: `colors` [N,H,W,K,3], or
    `atlas` [N*F,R,R,3] sampled at bary_coords (times ambient [N,3]); gradients to colors / atlas, dists and zbuf."""

    @staticmethod
    def forward(ctx, colors, atlas, dists, zbuf, bary, p2f, ambient, params):
        p2f, d, z = _i64c(p2f), _f32c(dists), _f32c(zbuf)
        K = p2f.shape[-1]
        P = p2f.numel() // K
        N, H, W = p2f.shape[:3]
        c = _f32c(colors) if colors is not None else None
        a = _f32c(atlas) if atlas is not None else None
        b = _f32c(bary) if atlas is not None else None
        am = _f32c(ambient) if ambient is not None else None
        R, Fp = (a.shape[1], a.shape[0]) if a is not None else (0, 0)
        rgba = torch.empty((N, H, W, 4), dtype=torch.float32, device=p2f.device)
        tune = _lib.tuning()[1]
        P_ = _lib.ptr
        _lib.call("acfm_softmax_rgb_blend", p2f.device, P_(p2f), P_(d), P_(z), P_(b), P_(c), P_(a), R, Fp, P_(am), P,
                  K, H * W, ctypes.byref(params), P_(rgba), _lib.tuning_ptr(tune))
        ctx.save_for_backward(p2f, d, z, b, c, a, am)
        ctx.cfg = (P, K, H * W, R, Fp, params, tune)
        ctx.set_materialize_grads(False)
        return rgba

    @staticmethod
    def backward(ctx, g):
        nig = ctx.needs_input_grad
        if g is None or not (nig[0] or nig[1] or nig[2] or nig[3]):
            return (None,) * 8
        p2f, d, z, b, c, a, am = ctx.saved_tensors
        P, K, HW, R, Fp, params, tune = ctx.cfg
        gc = torch.empty_like(c) if nig[0] else None
        ga = torch.empty_like(a) if nig[1] else None
        gd = torch.empty_like(d) if nig[2] else None
        gz = torch.empty_like(z) if nig[3] else None
        ws, nb = _det_ws(tune, a.numel(), a.device) if ga is not None else (None, 0)
        P_ = _lib.ptr
        _lib.call("acfm_softmax_rgb_blend_backward", p2f.device, P_(p2f), P_(d), P_(z), P_(b), P_(c), P_(a), R, Fp,
                  P_(am), P, K, HW, ctypes.byref(params), P_(_a16(g)), P_(gd), P_(gz), P_(gc), P_(ga), P_(ws), nb,
                  _lib.tuning_ptr(tune))
        return gc, ga, gd, gz, None, None, None, None


class _Interpolate(torch.autograd.Function):
    """interpolate_face_attributes (acfm_interpolate_face_attributes{,_backward}); gradients to bary and attributes."""

    @staticmethod
    def forward(ctx, bary, attrs, p2f):
        p2f, b, fa = _i64c(p2f), _f32c(bary), _f32c(attrs)
        K = p2f.shape[-1]
        P = p2f.numel() // K
        Fp, D = fa.shape[0], fa.shape[2]
        out = torch.empty(p2f.shape + (D,), dtype=torch.float32, device=p2f.device)
        tune = _lib.tuning()[1]
        _lib.call("acfm_interpolate_face_attributes", p2f.device, _lib.ptr(p2f), _lib.ptr(b), _lib.ptr(fa), P, K, Fp, D,
                  _lib.ptr(out), _lib.tuning_ptr(tune))
        ctx.save_for_backward(p2f, b, fa)
        ctx.cfg = (P, K, Fp, D, tune)
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    def backward(ctx, g):
        need_b, need_a = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if g is None or not (need_b or need_a):
            return None, None, None
        p2f, b, fa = ctx.saved_tensors
        P, K, Fp, D, tune = ctx.cfg
        gb = torch.empty_like(b) if need_b else None
        ga = torch.empty_like(fa) if need_a else None
        ws, nb = _det_ws(tune, fa.numel(), fa.device) if need_a else (None, 0)
        _lib.call("acfm_interpolate_face_attributes_backward", p2f.device, _lib.ptr(p2f), _lib.ptr(b), _lib.ptr(fa),
                  _lib.ptr(_f32c(g)), P, K, Fp, D, _lib.ptr(gb), _lib.ptr(ga), _lib.ptr(ws), nb, _lib.tuning_ptr(tune))
        return gb, ga, None


def sigmoid_alpha_blend(colors, fragments, blend_params, storage="f32"):
    """PyTorch3D 0.3.0 sigmoid_alpha_blend -> RGBA [N,H,W,4]: RGB = colors[..., 0, :] (1 where colors is None: the
    silhouette shader builds no ones_like tensor), A = 1 - prod_k (1 - sigmoid(-dists / sigma) [pix_to_face >= 0]).
    Differentiable with respect to colors [N,H,W,K,3] and fragments.dists."""
    _shade_storage(storage)
    p2f, zbuf, bary, dists = _frag_planes(fragments)
    if colors is not None and tuple(colors.shape) != tuple(p2f.shape) + (3,):
        raise ValueError("colors must be None or [N,H,W,K,3] = %s, got %s"
                         % (tuple(p2f.shape) + (3,), tuple(colors.shape)))
    _lib.require_gpu(p2f, zbuf, bary, dists, colors)
    if not blend_params.sigma > 0:
        raise ValueError("sigma must be > 0")
    return _SigmoidBlend.apply(colors, dists, p2f, float(blend_params.sigma))


def softmax_rgb_blend(colors, fragments, blend_params, znear=1.0, zfar=100.0, storage="f32"):
    """PyTorch3D 0.3.0 softmax_rgb_blend of colors [N,H,W,K,3] -> RGBA [N,H,W,4].
    Differentiable with respect to colors, fragments.dists and fragments.zbuf (the z_max path included)."""
    _shade_storage(storage)
    p2f, zbuf, bary, dists = _frag_planes(fragments)
    if tuple(colors.shape) != tuple(p2f.shape) + (3,):
        raise ValueError("colors must be [N,H,W,K,3] = %s, got %s" % (tuple(p2f.shape) + (3,), tuple(colors.shape)))
    _lib.require_gpu(p2f, zbuf, bary, dists, colors)
    return _SoftmaxBlend.apply(colors, None, dists, zbuf, None, p2f, None, blend_struct(blend_params, znear, zfar))


def atlas_softmax_blend(atlas, fragments, blend_params, ambient=None, znear=1.0, zfar=100.0, storage="f32"):
    """TexturesAtlas.sample_textures + an ambient-only Phong + softmax_rgb_blend in one pass (the reference's texture
    configuration): atlas [N,F,R,R,3] (or packed [N*F,R,R,3]) is sampled at fragments.bary_coords inside the kernel,
    times ambient [N,3] / [1,3] / [3] (a constant: no gradient) when given.  -> RGBA [N,H,W,4]; differentiable with
    respect to atlas, fragments.dists and fragments.zbuf (not bary_coords: the texel index is an integer)."""
    _shade_storage(storage)
    p2f, zbuf, bary, dists = _frag_planes(fragments)
    _lib.require_gpu(p2f, zbuf, bary, dists, atlas, ambient)
    if atlas.dim() == 5:
        atlas = atlas.reshape((-1,) + tuple(atlas.shape[2:]))
    if atlas.dim() != 4 or atlas.shape[1] != atlas.shape[2] or atlas.shape[3] != 3:
        raise ValueError("atlas must be [N,F,R,R,3] or [N*F,R,R,3] with 3 channels, got %s" % (tuple(atlas.shape),))
    N = p2f.shape[0]
    if ambient is not None:
        if ambient.requires_grad:
            raise ValueError("ambient is a constant of the fused atlas path (no gradient); use softmax_rgb_blend")
        ambient = ambient.detach().to(torch.float32).reshape(-1, 3)
        if ambient.shape[0] not in (1, N):
            raise ValueError("ambient must be [3], [1,3] or [N,3], got %s" % (tuple(ambient.shape),))
        ambient = ambient.expand(N, 3)
    return _SoftmaxBlend.apply(None, atlas, dists, zbuf, bary, p2f, ambient, blend_struct(blend_params, znear, zfar))


def interpolate_face_attributes(pix_to_face, barycentric_coords, face_attributes):
    """PyTorch3D 0.3.0 interpolate_face_attributes: face_attributes [F_packed,3,D] -> [N,H,W,K,D] = sum_i bary_i
    face_attributes[pix_to_face, i], 0 in empty slots.  Differentiable with respect to both float inputs."""
    K = int(pix_to_face.shape[-1])
    if K not in FRAGMENT_K:
        raise ValueError("faces_per_pixel=%d is not supported (one of %s)" % (K, FRAGMENT_K))
    if face_attributes.dim() != 3 or face_attributes.shape[1] != 3 or face_attributes.shape[2] < 1:
        raise ValueError("face_attributes must be [F,3,D], got %s" % (tuple(face_attributes.shape),))
    if tuple(barycentric_coords.shape) != tuple(pix_to_face.shape) + (3,):
        raise ValueError("barycentric_coords must be %s, got %s" % (tuple(pix_to_face.shape) + (3,),
                                                                    tuple(barycentric_coords.shape)))
    _lib.require_gpu(pix_to_face, barycentric_coords, face_attributes)
    return _Interpolate.apply(barycentric_coords, face_attributes, pix_to_face)


UV_PADDING_MODES = ("border", "zeros")


class _UvTexels(torch.autograd.Function):
    """TexturesUV.sample_textures (acfm_uv_texels{,_backward}); gradients to bary, faces_verts_uvs and
    maps, each formed only when asked for."""

    @staticmethod
    def forward(ctx, bary, fvuv, maps, p2f, align, pad):
        p2f, b, fv, m = _i64c(p2f), _f32c(bary), _f32c(fvuv), _f32c(maps)
        N, H, W, K = p2f.shape
        P = N * H * W
        Fp, Hm, Wm = fv.shape[0], m.shape[1], m.shape[2]
        out = torch.empty(p2f.shape + (3,), dtype=torch.float32, device=p2f.device)
        tune = _lib.tuning()[1]
        P_ = _lib.ptr
        _lib.call("acfm_uv_texels", p2f.device, P_(p2f), P_(b), P_(fv), P_(m), P, K, H * W, Fp, N, Hm, Wm, align, pad,
                  P_(out), _lib.tuning_ptr(tune))
        ctx.save_for_backward(p2f, b, fv, m)
        ctx.cfg = (P, K, H * W, Fp, N, Hm, Wm, align, pad, tune)
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    def backward(ctx, g):
        need_b, need_fv, need_m = ctx.needs_input_grad[:3]
        if g is None or not (need_b or need_fv or need_m):
            return (None,) * 6
        p2f, b, fv, m = ctx.saved_tensors
        P, K, HW, Fp, N, Hm, Wm, align, pad, tune = ctx.cfg
        gb = torch.empty_like(b) if need_b else None
        gfv = torch.empty_like(fv) if need_fv else None
        gm = torch.empty_like(m) if need_m else None
        n_acc = (fv.numel() if need_fv else 0) + (m.numel() if need_m else 0)
        ws, nb = _det_ws(tune, n_acc, p2f.device) if n_acc else (None, 0)
        P_ = _lib.ptr
        _lib.call("acfm_uv_texels_backward", p2f.device, P_(p2f), P_(b), P_(fv), P_(m), P_(_f32c(g)), P, K, HW, Fp, N,
                  Hm, Wm, align, pad, P_(gm), P_(gb), P_(gfv), P_(ws), nb, _lib.tuning_ptr(tune))
        return gb, gfv, gm, None, None, None


def uv_texels(pix_to_face, bary_coords, faces_verts_uvs, maps, align_corners=True, padding_mode="border"):
    """PyTorch3D 0.3.0 TexturesUV.sample_textures: pix_to_face [N,H,W,K], bary_coords [N,H,W,K,3],
    faces_verts_uvs [F_packed,3,2] (= verts_uvs[faces_uvs], mesh after mesh), maps [N,Hm,Wm,3] -> texels [N,H,W,K,3]
    = grid_sample(maps[n] flipped along its height, 2 uv - 1, bilinear, padding_mode, align_corners) at uv = sum_i
    bary_i faces_verts_uvs[f, i].  The map is read in place (no K-fold copy); empty slots are not zeroed, they hold
    the sample at uv = (0, 0).  Differentiable with respect to the three float inputs."""
    if pix_to_face.dim() != 4:
        raise ValueError("pix_to_face must be [N,H,W,K], got %s" % (tuple(pix_to_face.shape),))
    K = int(pix_to_face.shape[-1])
    if K not in FRAGMENT_K:
        raise ValueError("faces_per_pixel=%d is not supported (one of %s)" % (K, FRAGMENT_K))
    if tuple(bary_coords.shape) != tuple(pix_to_face.shape) + (3,):
        raise ValueError("bary_coords must be %s, got %s" % (tuple(pix_to_face.shape) + (3,),
                                                             tuple(bary_coords.shape)))
    if faces_verts_uvs.dim() != 3 or tuple(faces_verts_uvs.shape[1:]) != (3, 2) or faces_verts_uvs.shape[0] < 1:
        raise ValueError("faces_verts_uvs must be [F_packed,3,2], got %s" % (tuple(faces_verts_uvs.shape),))
    if maps.dim() != 4 or maps.shape[3] != 3 or maps.shape[0] != pix_to_face.shape[0]:
        raise ValueError("maps must be [N,Hm,Wm,3] with N = %d, got %s" % (pix_to_face.shape[0], tuple(maps.shape)))
    if padding_mode not in UV_PADDING_MODES:
        raise ValueError("padding_mode=%r is not supported (one of %s)" % (padding_mode, UV_PADDING_MODES))
    lo = 2 if align_corners else 1
    if min(maps.shape[1], maps.shape[2]) < lo or max(maps.shape[1], maps.shape[2]) > 16384:
        raise ValueError("maps must have sides in [%d, 16384]%s, got %s"
                         % (lo, " with align_corners=True" if align_corners else "", tuple(maps.shape)))
    if pix_to_face.numel() == 0:
        raise ValueError("pix_to_face is empty: %s" % (tuple(pix_to_face.shape),))
    for name, t in (("bary_coords", bary_coords), ("faces_verts_uvs", faces_verts_uvs), ("maps", maps)):
        if t.dtype != torch.float32:
            raise ValueError("%s must be float32 (half storage is not supported on the shader path), got %s"
                             % (name, t.dtype))
    _lib.require_gpu(pix_to_face, bary_coords, faces_verts_uvs, maps)
    return _UvTexels.apply(bary_coords, faces_verts_uvs, maps, pix_to_face, int(bool(align_corners)),
                           UV_PADDING_MODES.index(padding_mode))


# ------------------------------------------------------------------------------ texture
# atlas gradient: gather per face over the pixels of its box (acfm_tex_backward_faces, R <= 8) instead
# of one global float atomic per pixel and channel (acfm_tex_backward); both are kept and tested
TEX_BWD_GATHER = True


class _TexRender(torch.autograd.Function):
    """Atlas-textured render (acfm_tex_forward); fused=True: the render and its masked MSE against ref_img / ref_mask
    as one operator (acfm_tex_mse_forward / acfm_tex_mse_backward_faces), the image then carries no gradient.
    -> (loss or None, imgs, sil, pix_to_face)."""

    @staticmethod
    def forward(ctx, verts, faces, cams, atlas, ref_img, ref_mask, img_size, sigma, gamma, offset_z, f16, fused):
        _lib.require_gpu(verts, faces, cams, atlas, ref_img, ref_mask)
        v, c, a = _f32c(verts), _f32c(cams), _real(atlas, f16)   # (a float32 atlas is cast per call: hold it in half to spare that)
        N, V, _ = v.shape
        f = expand_faces(faces, N)
        F, H = f.shape[1], int(img_size)
        NA = a.shape[0] if a.dim() == 5 else 0
        if a.dim() != 5 or NA == 0 or N % NA != 0 or a.shape[1] != F or a.shape[2] != a.shape[3] or a.shape[4] != 3:
            raise ValueError("atlas must be [N,F,R,R,3] (or [N/G,F,R,R,3], shared by G hypotheses), got %s for "
                             "N=%d F=%d" % (tuple(a.shape), N, F))
        R = a.shape[2]
        ri = rm = loss = None
        RB = 0
        if fused:
            if R > 8:
                raise ValueError("tex_render_mse: atlas resolution R <= 8 (use tex_render + tex_mse beyond)")
            ri, rm = _real(ref_img, f16), _real(ref_mask, f16)
            RB = _ref_batch(N, ri, "tex_render_mse")
            if ri.shape[1:] != (3, H, H) or rm.reshape(-1, H, H).shape[0] != RB:
                raise ValueError("ref_img [N or N/G,3,H,H] and ref_mask [same batch,H,H]")
            rm = rm.reshape(RB, H, H)
            loss = torch.empty((N,), dtype=torch.float32, device=v.device)
        rdt = torch.float16 if f16 else torch.float32
        shared = _shared_setup(v, c, f, H, offset_z)
        if shared is not None:      # the workspace (and the tuning it was carved with) of the silhouette render
            ws, nb, ws_blur, tune, ent = shared
            ws_ready = _cover_taken(v.device, tune)
        else:
            ws, nb = _workspace(N, V, F, H, v.device)
            ws_blur, tune, ws_ready, ent = 0.0, _lib.tuning()[1], 0, None
        pf = _take_prefill(ent, N, H) if (ws_ready == 2 and not f16) else None
        if pf is not None:
            imgs, sil, p2f, tidx = pf          # their empty blocks were stored by the silhouette render
            ws_ready = 3
        else:
            imgs = torch.empty((N, 3, H, H), dtype=rdt, device=v.device)
            sil = torch.empty((N, H, H), dtype=rdt, device=v.device)
            p2f = torch.empty((N, H, H, 1), dtype=torch.int32 if f16 else torch.int64, device=v.device)
            tidx = torch.empty((N, H, H), dtype=torch.int32, device=v.device)
        tune = _lib.with_f16(tune, f16)
        P = _lib.ptr
        if fused:
            _lib.call("acfm_tex_mse_forward", v.device, P(v), P(f), P(c), P(a), P(ri), P(rm), RB, N, V, F, H, R,
                      float(sigma), float(gamma), float(offset_z), P(imgs), P(sil), P(p2f), P(tidx), P(loss), P(ws), nb,
                      ws_ready, float(ws_blur), NA, _lib.tuning_ptr(tune))
        else:
            _lib.call("acfm_tex_forward", v.device, P(v), P(f), P(c), P(a), N, V, F, H, R, float(sigma), float(gamma),
                      float(offset_z), P(imgs), P(sil), P(p2f), P(tidx), P(ws), nb, ws_ready, float(ws_blur), NA,
                      _lib.tuning_ptr(tune))
        ctx.save_for_backward(tidx, imgs, ri, rm)   # (imgs: to recognise a LazyGrad of this very image, at this version)
        ctx.cfg = (N, F, H, R, NA, V, RB)
        ctx.adt, ctx.tune, ctx.f16 = atlas.dtype, tune, f16
        ctx.ws = (ws, nb, float(ws_blur))   # face boxes: the gather form of the atlas gradient walks them
        ctx.mark_non_differentiable(*((imgs, sil, p2f) if fused else (sil, p2f)))
        ctx.set_materialize_grads(False)
        return loss, imgs, sil, p2f

    @staticmethod
    def backward(ctx, gloss, gimgs, _gs, _gp):
        tidx, imgs, ri, rm = ctx.saved_tensors
        N, F, H, R, NA, V, RB = ctx.cfg
        none = (None,) * 12
        if not ctx.needs_input_grad[3]:
            return none
        if gloss is not None:       # the fused operator
            pay = (imgs, ri, rm, RB, _f32c(gloss))
        elif type(gimgs) is LazyGrad and TEX_BWD_GATHER and R <= 8 and not ctx.f16:
            pay = gimgs.take("tex_mse", imgs)
        else:
            pay = None
        ws, nb, ws_blur = ctx.ws
        P = _lib.ptr
        ga = None
        if pay is not None:      # the texture MSE's gradient (a LazyGrad still unformed): the kernel forms it per pixel
            t0, ri, rm, rb, go = pay
            ga = torch.empty((NA, F, R, R, 3), dtype=torch.float32, device=t0.device)
            _lib.call("acfm_tex_mse_backward_faces", t0.device, P(t0), P(ri), P(rm), rb, P(go), P(tidx), P(ws), nb,
                      ws_blur, N, V, F, H, R, NA, P(ga), _lib.tuning_ptr(ctx.tune))
        elif gimgs is not None:
            g = _f32c(gimgs)
            ga = torch.empty((NA, F, R, R, 3), dtype=torch.float32, device=g.device)
            if TEX_BWD_GATHER and R <= 8:
                _lib.call("acfm_tex_backward_faces", g.device, P(g), P(tidx), P(ws), nb, ws_blur, N, V, F, H, R, NA, P(ga))
            else:
                _lib.call("acfm_tex_backward", g.device, P(g), P(tidx), N, F, H, R, NA, P(ga))
        # geometry / camera: integer texel lookup and K=1 blending send (numerically) no
        # gradient -- |d rgb / d dist| <= 1e-6 |texel| from the delta=1e-10 term.
        if ga is not None and ctx.adt != torch.float32:
            ga = ga.to(ctx.adt)
        return none[:3] + (ga,) + none[4:]


def tex_render(verts, faces, cams, atlas, img_size, sigma=1e-4, gamma=1e-4, offset_z=0.0, storage="f32"):
    """Atlas-textured hard render: -> (imgs [N,3,H,H], sil [N,H,H], pix_to_face [N,H,H,1]).
    atlas [N,F,R,R,3], or [N/G,F,R,R,3] when G hypotheses of every frame share the frame's
    texture (mesh n samples atlas n % (N/G); equivalent to atlas.repeat(G,1,1,1,1) without the
    copies, gradients of the G renders summed)."""
    return _TexRender.apply(verts, faces, cams, atlas, None, None, img_size, sigma, gamma, offset_z, _is_f16(storage),
                            False)[1:]


def tex_render_mse(verts, faces, cams, atlas, ref_img, ref_mask, img_size, sigma=1e-4, gamma=1e-4, offset_z=0.0,
                   storage="f32"):
    """Atlas-textured render and its masked MSE against reference images as ONE operator (opt-in; the drop-in pair is
    tex_render + tex_mse): -> (loss [N] = mean over (3,H,W) of (tex*mask - img*mask)^2, imgs [N,3,H,H] (no gradient),
    sil, pix_to_face).  Gradient flows from `loss` to the atlas.  ref_img / ref_mask: [N,...] or [N/G,...]."""
    return _TexRender.apply(verts, faces, cams, atlas, ref_img, ref_mask, img_size, sigma, gamma, offset_z,
                            _is_f16(storage), True)


def vertex_color_render(verts, faces, cams, verts_rgb, img_size, sigma=1e-4, gamma=1e-4, offset_z=0.0):
    """atlas=False path (per-vertex RGB, visualisation): forward only, no gradients."""
    _lib.require_gpu(verts, faces, cams, verts_rgb)
    v, c, col = _f32c(verts), _f32c(cams), _f32c(verts_rgb)
    N, V, _ = v.shape
    f = expand_faces(faces, N)
    F, H = f.shape[1], int(img_size)
    if col.dim() == 2:
        col = col[None]
    col = col.expand(N, V, 3).contiguous()
    imgs = torch.empty((N, 3, H, H), dtype=torch.float32, device=v.device)
    sil = torch.empty((N, H, H), dtype=torch.float32, device=v.device)
    p2f = torch.empty((N, H, H, 1), dtype=torch.int64, device=v.device)
    nb = _lib.lib().acfm_raster_workspace_bytes(N, V, F, H) + 4 * N * H * H
    ws = torch.empty(nb, dtype=torch.uint8, device=v.device)
    _lib.call("acfm_vertex_color_forward", v.device, _lib.ptr(v), _lib.ptr(f), _lib.ptr(c), _lib.ptr(col), N, V, F, H,
              float(sigma), float(gamma), float(offset_z), _lib.ptr(imgs), _lib.ptr(sil), _lib.ptr(p2f), _lib.ptr(ws),
              nb, 0, 0.0, _lib.tuning()[0])
    return imgs, sil, p2f


# ------------------------------------------------------------------------------ deferred loss terms
# The three per-mesh loss sums of a step (mask_losses, tex_mse, bds_loss_per_mesh) are short launches, and the step
# ends in combine_losses over them.  Like LazyPixToFace and LazyGrad, their forward is deferred: the operator allocates
# its output, notes a job (arguments, inputs and the inputs' versions) and returns the output as a PendingTerm.
# combine_losses launches the pending jobs among its terms and the total as ONE kernel (acfm_step_losses_forward).
# Any other use of a PendingTerm first runs the launch the operator would have made (flush): torch functions on it
# (arithmetic, indexing, .item(), .cpu(), printing, another operator saving it), its own backward,
# invalidate_setups() / graph_replay(), flush_pending_losses().  What a flush refuses: an input written in place
# since the call (RuntimeError naming it), and a term deferred inside a hipGraph capture that ended without using it
# (the launch can no longer be recorded).  So that this does not happen, graphed.GraphedStep flushes before it ends
# its capture, and inside ANY capture a term is deferred only if the last term of its kind on the device left in a
# one-launch combine_losses -- which the eager warm-up calls that precede every capture have shown by then (the way
# the cover flag above follows what the texture renders do); a term that a capture returns unread is launched where
# it is called.  With a capture of your own that differs from its warm-up, call flush_pending_losses() before
# leaving it.  Terms are not deferred on the worker threads nn.DataParallel runs its replicas on (their outputs are
# gathered by code that does not look at the type).
_DEFER = [True]
_PENDING = weakref.WeakSet()
_FUSED_LAST = {}         # (device index, kind) -> the last job of that kind was launched with others by combine_losses


@contextlib.contextmanager
def defer_losses(on=True):
    """with ops.defer_losses(False): every loss term is launched where it is called (no PendingTerm)."""
    flush_pending_losses()
    with _LOCK:
        old, _DEFER[0] = _DEFER[0], bool(on)
    try:
        yield
    finally:
        flush_pending_losses()
        with _LOCK:
            _DEFER[0] = old


def _deferring(device=None, kind=None):
    if not _DEFER[0] or threading.current_thread() is not threading.main_thread():
        return False
    if device is not None and torch.cuda.is_current_stream_capturing():
        return _FUSED_LAST.get((device.index, kind), False)
    return True


def flush_pending_losses():
    """Launch every loss term that is still deferred (each by its own kernel)."""
    with _LOCK:
        jobs = list(_PENDING)
    for j in jobs:
        j.flush()


def launch_pending_together(terms):
    """The pending terms among `terms` (at most one of each kind; same batch, stream and capture) as ONE launch
    without a total -- what combine_losses does for its terms, for callers that add the terms up themselves."""
    jobs = []
    for t in terms:
        j = t._job if type(t) is PendingTerm else None
        if j is not None and not j.done and j not in jobs:
            if any(k.kind == j.kind or k.N != j.N or k.device != j.device or k.stream != j.stream or k.cid != j.cid
                   for k in jobs):
                raise ValueError("launch_pending_together: one term of each kind, on the same batch, stream and capture")
            jobs.append(j)
    if jobs:
        if jobs[0].stream != torch.cuda.current_stream(jobs[0].device):
            raise ValueError("launch_pending_together: call it on the stream the terms were called on")
        _launch_step_tail(jobs, None)


class _PendingJob:
    """A loss term whose launch has not been issued: kind 'mask' / 'tex' / 'bds', the output tensor(s), the inputs as
    (name, tensor, version at the call), `launch` (the operator's own entry point) and `fill` (-> the job structure of
    acfm_step_losses_forward)."""

    def __init__(self, kind, what, out, N, inputs, launch, fill, sizes):
        self.kind, self.what, self.out, self.N = kind, what, out, N
        self.inputs = [(name, t, t._version) for name, t in inputs if t is not None]
        self.launch, self.fill, self.sizes = launch, fill, sizes
        self.device = out.device
        self.stream = torch.cuda.current_stream(self.device)
        self.cid = _capture_id(self.device)
        self.done = False
        with _LOCK:
            _PENDING.add(self)

    def check(self):
        """Raises unless the job can still be launched on what its operator was called with."""
        for name, t, version in self.inputs:
            if t._version != version:
                raise RuntimeError("%s: `%s` was written in place after the call and before its deferred launch "
                                   "(combine_losses, or the first use of the result); the loss is not computed on "
                                   "changed data -- use ops.defer_losses(False) or write after the result is used"
                                   % (self.what, name))
        with torch.cuda.stream(self.stream):
            cid = _capture_id(self.device)
        if cid != self.cid:
            raise RuntimeError("%s: called inside a hipGraph capture that ended before its deferred launch was "
                               "recorded; call ops.flush_pending_losses() before leaving the capture" % self.what
                               if self.cid else
                               "%s: called before a hipGraph capture and first used inside it; call "
                               "ops.flush_pending_losses() before the capture begins" % self.what)

    def __del__(self):
        if not getattr(self, "done", True):   # dropped unread: nothing was launched for it, certainly not with others
            _FUSED_LAST[(self.device.index, self.kind)] = False

    def taken(self, fused=False):
        _FUSED_LAST[(self.device.index, self.kind)] = fused
        self.done = True
        self.launch = self.fill = None
        self.inputs = []
        with _LOCK:
            _PENDING.discard(self)

    def flush(self):
        if self.done:
            return
        self.check()             # (a job that cannot be launched stays pending: every use of its term raises)
        self.done = True
        try:
            cur = torch.cuda.current_stream(self.device)
            with torch.cuda.stream(self.stream):   # where the call was made: its inputs are ordered there
                self.launch()
            if cur != self.stream:
                cur.wait_stream(self.stream)
        finally:
            self.taken()


def _pending_terms(args):
    found = []

    def walk(x):
        if type(x) is PendingTerm:
            found.append(x)
        elif isinstance(x, (list, tuple)):
            for y in x:
                walk(y)
        elif isinstance(x, dict):
            for y in x.values():
                walk(y)
    walk(args)
    return found


class PendingTerm(torch.Tensor):
    """The output of a deferred loss operator (see above): a tensor on the operator's output storage, with the
    operator's grad_fn, whose values exist once its job has been launched.  Reading it in any way launches the job."""

    @staticmethod
    def __new__(cls, out, job):
        r = torch.Tensor._make_subclass(cls, out)
        r._job = job
        return r

    @property
    def is_pending(self):
        return not self._job.done

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        if func not in _PENDING_META:
            for t in _pending_terms((args, kwargs)):
                t._job.flush()
        with torch._C.DisableTorchFunctionSubclass():
            return func(*args, **kwargs)


# what can be asked of a PendingTerm without its values
_PENDING_META = {getattr(torch.Tensor, n).__get__ for n in
                 ("shape", "device", "dtype", "requires_grad", "grad_fn", "_version", "is_cuda", "is_leaf", "ndim",
                  "layout", "names", "is_sparse", "is_quantized", "is_meta", "output_nr", "_base", "grad")}
_PENDING_META |= {torch.Tensor.dim, torch.Tensor.size, torch.Tensor.numel, torch.Tensor.nelement, torch.Tensor.data_ptr,
                  torch.Tensor.stride, torch.Tensor.is_contiguous, torch.Tensor.element_size, torch.Tensor.get_device,
                  torch.Tensor.is_floating_point, torch.Tensor.storage_offset, torch.Tensor.ndimension,
                  torch.Tensor.is_complex}


def _raw(t):
    """A PendingTerm's storage as a plain tensor, without launching its job."""
    return t._job.out if type(t) is PendingTerm else t


def _step_scratch(device, N, hw_mask, hw_tex, S):
    words = ctypes.c_size_t(0)
    need = int(_lib.lib().acfm_step_losses_ws(N, hw_mask, hw_tex, S, ctypes.byref(words)))
    return _row_scratch(device, "step_tail", int(words.value), need)


def _launch_step_tail(jobs, total):
    """The pending `jobs` (at most one of each kind, same N, device, stream and capture) and, if total =
    (term tensors [N,C], cols, weights, out) is given, the weighted total, as one acfm_step_losses_forward."""
    dev, N = jobs[0].device, jobs[0].N
    for j in jobs:
        j.check()
    by_kind = {j.kind: j for j in jobs}
    keep = []
    structs = {}
    for kind in ("mask", "tex", "bds"):
        j = by_kind.get(kind)
        if j is not None:
            structs[kind] = j.fill()
            keep.append(structs[kind])
    sz = {k: (by_kind[k].sizes if k in by_kind else 0) for k in ("mask", "tex", "bds")}
    with torch.cuda.device(dev):
        tk, part, nf = _step_scratch(dev, N, sz["mask"], sz["tex"], sz["bds"])
    tot = None
    if total is not None:
        ts, cols, weights, out = total
        ptrs = (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        tot = _lib.StepTotalJob(ctypes.cast(ptrs, ctypes.c_void_p), ctypes.cast(cols, ctypes.c_void_p),
                                ctypes.cast(weights, ctypes.c_void_p), len(ts), out.data_ptr())
        keep.append(ptrs)

    def ref(x):
        return ctypes.cast(ctypes.pointer(x), ctypes.c_void_p) if x is not None else None
    for j in jobs:
        j.done = True
    try:
        _lib.call("acfm_step_losses_forward", dev, ref(structs.get("mask")), ref(structs.get("tex")),
                  ref(structs.get("bds")), ref(tot), N, _lib.ptr(tk), _lib.ptr(part), nf)
    finally:
        for j in jobs:
            j.taken(fused=True)


# ------------------------------------------------------------------------------ mask losses
def _ref_batch(N, ref, what):
    """References (ground-truth masks, images, boundary points) may be given once per frame for the G
    hypotheses rendered of it: [N/G, ...] against N predictions, prediction n <-> reference n % (N/G)
    (= the trainer's ref.repeat(G, ...) without the copies)."""
    RB = ref.shape[0]
    if RB <= 0 or N % RB != 0:
        raise ValueError("%s: %d references for %d predictions (must divide)" % (what, RB, N))
    return RB


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
            _lib.call("acfm_mask_losses_ws", m.device, _lib.ptr(m), _lib.ptr(g), _lib.ptr(e), N, HW, RB, _lib.ptr(out),
                      _lib.ptr(tk), _lib.ptr(part), nf)
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
            _lib.call("acfm_mask_losses_backward", m.device, _lib.ptr(m), _lib.ptr(g), _lib.ptr(e), _lib.ptr(go), N, HW,
                      rb, _lib.ptr(gm))
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
            _lib.call("acfm_tex_mse_ws", t.device, _lib.ptr(t), _lib.ptr(i), _lib.ptr(m), N, HW, RB, _lib.ptr(out),
                      _lib.ptr(tk), _lib.ptr(part), nf)
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
            _lib.call("acfm_tex_mse_backward", t.device, _lib.ptr(t), _lib.ptr(i), _lib.ptr(m), _lib.ptr(g), N, HW, rb,
                      _lib.ptr(gt))
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
        _lib.call("acfm_combine_losses", total.device, ptrs, ctx.args[0], ctx.args[1], len(ts), N, _lib.ptr(total))
        return total

    @staticmethod
    def backward(ctx, go):
        cols, w, nt, N, shapes = ctx.args
        g = _f32c(go).reshape(1)
        need = ctx.needs_input_grad[1:]
        outs = [torch.empty((N, cols[i]), dtype=torch.float32, device=g.device) if need[i] else None
                for i in range(nt)]
        ptrs = (ctypes.c_void_p * nt)(*[(o.data_ptr() if o is not None else None) for o in outs])
        _lib.call("acfm_combine_losses_backward", g.device, _lib.ptr(g), ptrs, cols, w, nt, N)
        return (None,) + tuple(o.reshape(shapes[i]) if o is not None else None for i, o in enumerate(outs))


def combine_losses(terms, weights):
    """(1/N) sum_n sum_t sum_c w[t][c] * terms[t][n, c] -> scalar: the weighted total of per-mesh loss
    vectors and its batch mean (multiframe/main.py:716-765) as one launch each way.  terms: up to 4
    tensors [N] or [N, C<=4] (e.g. the [N,4] output of mask_losses as it is); weights: one float per
    column, flattened term by term."""
    return _Combine.apply(tuple(float(w) for w in weights), *terms)


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
        _lib.call("acfm_hypothesis_total", dev, ptrs, w, ag, aw, nt, G, N, _lib.ptr(total), _lib.ptr(probs),
                  _lib.ptr(aux[0]), _lib.ptr(aux[1]), _lib.ptr(out))
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
        _lib.call("acfm_hypothesis_total_backward", g.device, _lib.ptr(g), _lib.ptr(probs), w, nt, G, N, ptrs)
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
        _lib.call("acfm_texture_cycle", x.device, _lib.ptr(x), B, int(T), F, R, _lib.ptr(scratch), _lib.ptr(loss))
        ctx.save_for_backward(x, scratch)
        ctx.cfg = (B, int(T), F, R, textures.dtype)
        return loss

    @staticmethod
    def backward(ctx, go):
        x, scratch = ctx.saved_tensors
        B, T, F, R, dt = ctx.cfg
        g = _f32c(go).reshape(1)
        gx = torch.empty_like(x)
        _lib.call("acfm_texture_cycle_backward", x.device, _lib.ptr(x), _lib.ptr(scratch), _lib.ptr(g), B, T, F, R,
                  _lib.ptr(gx))
        return (gx if dt == torch.float32 else gx.to(dt)), None


def texture_cycle(textures, num_frames):
    """The texture temporal-consistency term of ShapeTrainer.forward as written there (multiframe/main.py:705-711):
    atlases [B*T,F,R,R,3] -> scalar; two launches forward, one backward (fixed summation order)."""
    return _TexCycle.apply(textures, int(num_frames))


# ------------------------------------------------------------------------------ boundary loss
def visible_vertices(pix_to_face, faces, nv):
    """[N,H,W,K] i64 (slot 0 read) x faces [N,F,3] -> uint8 [N,nv].  A pix_to_face tensor that
    comes straight from sil_render / hard_raster carries the bitmap already (fused into the
    raster kernel); any other tensor goes through the stand-alone kernel."""
    fused = getattr(pix_to_face, "_acfm_vis", None)
    if fused is not None and fused.shape == (pix_to_face.shape[0], nv):
        return fused
    if isinstance(pix_to_face, LazyPixToFace) and not pix_to_face.is_materialized:
        pix_to_face = pix_to_face[..., :1]          # the stand-alone kernel reads slot 0 only
    _lib.require_gpu(pix_to_face, faces)
    p = pix_to_face.detach().to(torch.int64).contiguous()
    N, K = p.shape[0], p.shape[-1]
    HW = p[0].numel() // K
    f = expand_faces(faces, N)
    vis = torch.empty((N, nv), dtype=torch.uint8, device=p.device)
    _lib.call("acfm_visible_vertices", p.device, _lib.ptr(p), _lib.ptr(f), N, nv, f.shape[1], HW, K, _lib.ptr(vis))
    return vis


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
            _lib.call("acfm_bds_loss_ws", v.device, _lib.ptr(v), _lib.ptr(b), _lib.ptr(vz), N, V, P, RB,
                      _lib.ptr(loss), _lib.ptr(arg), _lib.ptr(tk), _lib.ptr(part), nf)
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
        _lib.call("acfm_bds_loss_backward", v.device, _lib.ptr(v), _lib.ptr(b), _lib.ptr(arg), _lib.ptr(g), N, V, P,
                  ctx.rb, _lib.ptr(gv))
        return gv, None, None


class _BdsLossSel(torch.autograd.Function):
    """_BdsLoss with every point read through a slot list (acfm_bds_loss_sel_ws): no gathered copy of the points."""

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
            _lib.call("acfm_bds_loss_sel_ws", v.device, _lib.ptr(v), _lib.ptr(b), _lib.ptr(vz), _lib.ptr(s),
                      N, V, P, RB, rows, S, _lib.ptr(loss), _lib.ptr(arg), _lib.ptr(tk), _lib.ptr(part), nf)
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
        _lib.call("acfm_bds_loss_sel_backward", v.device, _lib.ptr(v), _lib.ptr(b), _lib.ptr(s), _lib.ptr(arg),
                  _lib.ptr(g), N, V, P, ctx.rb, rows, S, _lib.ptr(gv))
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
    _lib.call("acfm_boundary_subset", state.device, _lib.ptr(state), _lib.ptr(counts), nc, rows, int(P),
              int(n_samples), _lib.ptr(sel))
    return sel


# ------------------------------------------------------------------------------ mesh priors
def cot_laplacian(verts, faces):
    """Dense cot Laplacian L [V,V] of one mesh (verts [V,3], faces [F,3]); constant (no grad)."""
    _lib.require_gpu(verts, faces)
    v = _f32c(verts)
    f = faces.detach().to(torch.int64).contiguous()
    V, F = v.shape[0], f.shape[0]
    L = torch.empty((V, V), dtype=torch.float32, device=v.device)
    _lib.call("acfm_cot_laplacian", v.device, _lib.ptr(v), _lib.ptr(f), V, F, _lib.ptr(L))
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
        _lib.call("acfm_laplacian_smoothing", v.device, _lib.ptr(v), _lib.ptr(c), _lib.ptr(w), P, F, int(method),
                  int(vpm), int(fpm), _lib.ptr(loss), _lib.ptr(state))
        ctx.save_for_backward(c, state)
        ctx.cfg = (P, F, int(method), int(vpm), int(fpm))
        return loss

    @staticmethod
    def backward(ctx, go):
        c, state = ctx.saved_tensors
        P, F, method, vpm, fpm = ctx.cfg
        g = _f32c(go).reshape(1)
        gv = torch.empty((P, 3), dtype=torch.float32, device=g.device)
        _lib.call("acfm_laplacian_smoothing_backward", g.device, _lib.ptr(c), _lib.ptr(state), _lib.ptr(g), P, F,
                  method, vpm, fpm, _lib.ptr(gv))
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
        _lib.call("acfm_edge_rigidity", v.device, _lib.ptr(v), _lib.ptr(e), _lib.ptr(vt), _lib.ptr(et), e.shape[0],
                  _lib.ptr(loss))
        ctx.save_for_backward(v, e, vt, et)
        ctx.vpm = int(vpm)
        return loss

    @staticmethod
    def backward(ctx, go):
        v, e, vt, et = ctx.saved_tensors
        g = _f32c(go).reshape(1)
        gv = torch.empty_like(v) if ctx.needs_input_grad[0] else None
        gvt = torch.empty_like(vt) if ctx.needs_input_grad[2] else None
        _lib.call("acfm_edge_rigidity_backward", g.device, _lib.ptr(v), _lib.ptr(e), _lib.ptr(vt), _lib.ptr(et),
                  e.shape[0], v.shape[0], vt.shape[0], ctx.vpm, _lib.ptr(g), _lib.ptr(gv), _lib.ptr(gvt))
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
        _lib.call("acfm_chamfer", a.device, _lib.ptr(a), _lib.ptr(b), _lib.ptr(xl), _lib.ptr(yl), N, P1, P2,
                  _lib.ptr(sums), _lib.ptr(ix), _lib.ptr(iy), _lib.ptr(tk), _lib.ptr(part), nf)
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
        _lib.call("acfm_chamfer_backward", a.device, _lib.ptr(a), _lib.ptr(b), _lib.ptr(xl), _lib.ptr(yl), _lib.ptr(ix),
                  _lib.ptr(iy), _lib.ptr(g), N, P1, P2, _lib.ptr(ga), _lib.ptr(gb))
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
        _lib.call("acfm_edge_length_loss", v.device, _lib.ptr(v), _lib.ptr(e), _lib.ptr(w), P, E, float(target),
                  _lib.ptr(loss), _lib.ptr(tk), _lib.ptr(part), nf)
        ctx.save_for_backward(v, e, w)
        ctx.target = float(target)
        return loss

    @staticmethod
    def backward(ctx, go):
        v, e, w = ctx.saved_tensors
        g = _f32c(go).reshape(1)
        gv = torch.empty_like(v)
        _lib.call("acfm_edge_length_loss_backward", v.device, _lib.ptr(v), _lib.ptr(e), _lib.ptr(w), _lib.ptr(g),
                  v.shape[0], e.shape[0], ctx.target, _lib.ptr(gv))
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
        _lib.call("acfm_normal_consistency", v.device, _lib.ptr(v), _lib.ptr(q), _lib.ptr(w), P, Q, _lib.ptr(loss),
                  _lib.ptr(tk), _lib.ptr(part), nf)
        ctx.save_for_backward(v, q, w)
        return loss

    @staticmethod
    def backward(ctx, go):
        v, q, w = ctx.saved_tensors
        g = _f32c(go).reshape(1)
        gv = torch.empty_like(v)
        _lib.call("acfm_normal_consistency_backward", v.device, _lib.ptr(v), _lib.ptr(q), _lib.ptr(w), _lib.ptr(g),
                  v.shape[0], q.shape[0], _lib.ptr(gv))
        return gv, None, None


def normal_consistency_sum(verts_packed, quads, qweight):
    """sum_q qweight[q] (1 - cos(n0, n1)) over the pairs of faces (a, b, c), (a, b, d) on an edge: quads [Q,4] =
    (a, b, c, d), Q > 0 (Meshes.normal_pairs_packed() builds them)."""
    return _NormalConsistency.apply(verts_packed, quads, qweight)


# ------------------------------------------------------------------------------ geodesic handles (csrc/acfm_geodesic.hip)
GEODESIC_MAX_STEINER = 20        # ACFM_GEODESIC_MAX_STEINER: 3 m + 3 boundary nodes of a face fit one wave
GEODESIC_LDS_MAX = 153600        # ACFM_GEODESIC_LDS_MAX


def geodesic_max_steiner(V, E):
    """The largest steiner count whose graph (V + m E nodes, 4 bytes each) fits one workgroup's LDS; -1 if none does."""
    fits = [m for m in range(GEODESIC_MAX_STEINER + 1)
            if 0 < int(_lib.lib().acfm_geodesic_lds_bytes(int(V), int(E), m)) <= GEODESIC_LDS_MAX]
    return max(fits) if fits else -1


GEODESIC_MEMORY = ("lds", "device", "auto")


def geodesic_memory(memory):
    """`memory` of geodesic_distances, validated: one of "lds", "device", "auto"."""
    if memory not in GEODESIC_MEMORY:
        raise ValueError('memory must be one of "lds", "device", "auto", got %r' % (memory,))
    return memory


def geodesic_device_workgroups(items, max_workgroups=None):
    """The grid of the device-memory kernel for `items` = S N (source, mesh) pairs: min(items, max_workgroups),
    max_workgroups None = two per CU of the current device."""
    one = int(_lib.lib().acfm_geodesic_workspace_bytes(1, 1, 0, 0, 1, 1))
    return int(_lib.lib().acfm_geodesic_workspace_bytes(1, 1, 0, 0, int(items), int(max_workgroups or 0))) // one


def geodesic_distances(verts, faces, steiner=15, sources=None, memory="lds", max_workgroups=None):
    """Surface distances between the vertices of a mesh, for the handle weights of mesh_net.py:69-85, 523-544 (there
    gdist.local_gdist_matrix): shortest paths on the edge-Steiner graph -- `steiner` = m points on every edge, inside
    every face all pairs of its 3 + 3 m boundary nodes joined by their Euclidean distance.  An upper bound of the exact
    geodesic (DESIGN.md "Geodesic handles": under 0.2 % at the default m = 15), +inf between components, 0 on the
    diagonal; the same bits on every run.
    verts [V,3] or [N,V,3] float32 on the GPU, faces [F,3] (one topology for all N), sources: None (all V vertices) or
    S vertex ids (a sequence or an integer tensor; any order, repeats allowed) -> [S,V] or [N,S,V] float32, detached (the
    reference computes these in numpy).
    memory = "lds": one launch, one workgroup per (source, mesh), the graph in LDS: a graph of more than 153,584 / 4
    nodes is refused with the largest steiner count that fits.  "device": the same relaxation with the distances in a
    per-call workspace (one row of V + m E floats per resident workgroup), any graph, the same bits; a persistent grid
    of min(S N, max_workgroups) workgroups, max_workgroups None = two per CU.  "auto": "lds" where the graph fits,
    else "device".
    The int32 edge tables are built once per faces tensor (Meshes.geodesic_tables_packed) and `sources` is uploaded per
    call: inside a graph capture the op runs only when the tables exist and `sources` is None or an int32 tensor on the
    device, and it raises otherwise."""
    from .pytorch3d_shim.structures import Meshes
    if not (torch.is_tensor(verts) and torch.is_tensor(faces)):
        raise ValueError("geodesic_distances: verts and faces must be tensors (handles.geodesic_distance_matrix takes arrays)")
    _lib.require_gpu(verts, faces)
    if verts.dim() not in (2, 3) or verts.shape[-1] != 3 or verts.shape[-2] < 1 or verts.shape[0] < 1:
        raise ValueError("geodesic_distances: verts [V,3] or [N,V,3] expected, got %s" % (tuple(verts.shape),))
    if verts.dtype != torch.float32:
        raise ValueError("geodesic_distances: verts must be float32, got %s" % verts.dtype)
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] < 1 or faces.dtype.is_floating_point:
        raise ValueError("geodesic_distances: faces [F,3] of integers expected (one topology), got %s %s"
                         % (faces.dtype, tuple(faces.shape)))
    if faces.device != verts.device:
        raise ValueError("geodesic_distances: verts are on %s, faces on %s" % (verts.device, faces.device))
    m = int(steiner)
    if m != steiner or not 0 <= m <= GEODESIC_MAX_STEINER:
        raise ValueError("steiner must be an integer in [0, %d] (3 steiner + 3 nodes per face, one wave), got %r"
                         % (GEODESIC_MAX_STEINER, steiner))
    geodesic_memory(memory)
    if max_workgroups is not None and (int(max_workgroups) != max_workgroups or int(max_workgroups) < 1):
        raise ValueError("max_workgroups must be None or a positive integer, got %r" % (max_workgroups,))
    dev = verts.device
    v = verts.detach().contiguous()
    batched = v.dim() == 3
    v3 = v if batched else v[None]
    N, V = v3.shape[0], v3.shape[1]
    capturing = torch.cuda.is_current_stream_capturing()
    mesh = Meshes(verts=[v3[0]], faces=[faces])
    if not mesh.has_geodesic_tables():
        if capturing:
            raise RuntimeError("geodesic_distances cannot build its edge tables inside a graph capture: call it once on "
                               "this faces tensor before capturing")
        lo, hi = int(faces.min()), int(faces.max())
        if lo < 0 or hi >= V:
            raise ValueError("faces hold vertex ids in [%d, %d], the mesh has %d vertices" % (lo, hi, V))
    f32, e32, fe32 = mesh.geodesic_tables_packed()
    F_, E = f32.shape[0], e32.shape[0]
    with torch.cuda.device(dev):
        need = int(_lib.lib().acfm_geodesic_lds_bytes(V, E, m))
    fits = 0 < need <= GEODESIC_LDS_MAX
    if memory == "lds" and not fits:
        raise ValueError("geodesic_distances: %d vertices + %d x %d edge points need %d bytes of LDS, a workgroup has %d; "
                         "the largest steiner that fits this mesh is %d" % (V, m, E, 16 + 4 * (V + m * E),
                                                                           GEODESIC_LDS_MAX, geodesic_max_steiner(V, E)))
    src = None
    if sources is not None:
        if torch.is_tensor(sources) and sources.is_cuda and sources.dtype == torch.int32:
            src = sources.detach().contiguous()
        elif capturing:
            raise RuntimeError("geodesic_distances inside a graph capture: sources must be None or an int32 tensor on "
                               "the device (anything else is uploaded)")
        else:
            src = torch.as_tensor(sources).detach().to(device=dev, dtype=torch.int32).contiguous()
        if src.dim() != 1 or src.numel() < 1 or src.device != dev:
            raise ValueError("sources: S >= 1 vertex ids on %s expected, got %s on %s" % (dev, tuple(src.shape), src.device))
        if not capturing:
            lo, hi = int(src.min()), int(src.max())
            if lo < 0 or hi >= V:
                raise ValueError("sources hold vertex ids in [%d, %d], the mesh has %d vertices" % (lo, hi, V))
    S = V if src is None else src.shape[0]
    out = torch.empty((N, S, V), dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    if memory == "lds" or (memory == "auto" and fits):
        _lib.call("acfm_geodesic_distances", dev, _lib.ptr(v3), _lib.ptr(f32), _lib.ptr(e32), _lib.ptr(fe32), N, V, F_, E,
                  m, _lib.ptr(src), S, _lib.ptr(out), _lib.ptr(status))
    else:
        cap = int(max_workgroups or 0)
        with torch.cuda.device(dev):
            ws_bytes = int(_lib.lib().acfm_geodesic_workspace_bytes(N, V, E, m, S, cap))
        if ws_bytes == 0:
            raise ValueError("geodesic_distances: no workspace size for N = %d, V = %d, E = %d, steiner = %d, S = %d"
                             % (N, V, E, m, S))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        _lib.call("acfm_geodesic_distances_dev", dev, _lib.ptr(v3), _lib.ptr(f32), _lib.ptr(e32), _lib.ptr(fe32), N, V,
                  F_, E, m, _lib.ptr(src), S, _lib.ptr(out), _lib.ptr(status), cap, _lib.ptr(ws), ws_bytes)
    if not capturing:       # (a captured call cannot read it: a workgroup that gave up leaves a row of NaN)
        st = int(status.item())
        if st:
            raise RuntimeError("acfm_geodesic_distances: %s" % {
                1: "no fixed point after V + m E sweeps",
                2: "a source outside [0, V)"}.get(st, "status %d" % st))
    return out if batched else out[0]


# ------------------------------------------------------------------------------ texture head (csrc/acfm_uvatlas.hip)
class UVAtlasTable:
    """What uv_atlas needs of a constant sampler (uv_atlas_table builds it): the float32 sampler [F',T,T,2] and, on the
    GPU, the per-pixel tap lists of the backward -- pix_start [Hu*Wu+1] i32, pix_taps [n_entries] i32 (sample * 4 +
    corner, ascending inside a pixel: the summation order)."""

    def __init__(self, sampler, Hu, Wu, pix_start=None, pix_taps=None):
        self.sampler, self.Hu, self.Wu = sampler, int(Hu), int(Wu)
        self.Fp, self.T = int(sampler.shape[0]), int(sampler.shape[1])
        self.pix_start, self.pix_taps = pix_start, pix_taps
        self.n_entries = 0 if pix_taps is None else int(pix_taps.shape[0])

    @property
    def device(self):
        return self.sampler.device


def _uv_table_from_taps(tap_pixel, n_pixels):
    """tap_pixel [n_samples,4] (pixel of each sample's four taps, -1 = outside) -> (pix_start [n_pixels+1] i32,
    pix_taps [count] i32): pixel p owns pix_taps[pix_start[p]:pix_start[p+1]], entries sample * 4 + corner in ascending
    order (a stable sort by pixel of the entries in their own order)."""
    flat = tap_pixel.reshape(-1).to(torch.int64)
    entry = torch.nonzero(flat >= 0).reshape(-1)
    pix = flat[entry]
    if pix.numel() and int(pix.max()) >= n_pixels:
        raise ValueError("tap_pixel holds pixel %d, the image has %d" % (int(pix.max()), n_pixels))
    order = torch.sort(pix, stable=True).indices
    pix_start = torch.zeros(n_pixels + 1, dtype=torch.int32, device=flat.device)
    pix_start[1:] = torch.cumsum(torch.bincount(pix, minlength=n_pixels), 0)
    return pix_start, entry[order].to(torch.int32)


def uv_atlas_table(uv_sampler, Hu, Wu):
    """The table of uv_atlas for a sampler [F',T,T,2] (utils/mesh.py:206-232, any float type; kept as float32 as
    mesh_net.py:559 keeps it) and a UV image size, on the sampler's device.  Build it once per model and device, outside
    any graph capture (it sorts and sizes its lists on the host's say).  On the GPU it runs acfm_uv_atlas_taps, so the
    lists hold exactly the taps the forward kernel takes."""
    Hu, Wu = int(Hu), int(Wu)
    if uv_sampler.dim() != 4 or uv_sampler.shape[1] != uv_sampler.shape[2] or uv_sampler.shape[3] != 2 \
            or uv_sampler.shape[0] < 1 or uv_sampler.shape[1] < 1:
        raise ValueError("uv_sampler: [F',T,T,2] with F', T >= 1 expected, got %s" % (tuple(uv_sampler.shape),))
    if Hu < 2:
        raise ValueError("Hu must be at least 2 (align_corners=True spreads [-1, 1] over Hu - 1 pixels), got %d" % Hu)
    if Wu < 2:
        raise ValueError("Wu must be at least 2 (align_corners=True spreads [-1, 1] over Wu - 1 pixels), got %d" % Wu)
    if uv_sampler.is_cuda and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("uv_atlas_table cannot run inside a graph capture: build the table with uv_atlas_table "
                           "(or run the UVAtlasSampler once) before capturing")
    s = uv_sampler.detach().to(torch.float32).contiguous()
    if not bool(torch.isfinite(s).all()):
        raise ValueError("uv_sampler holds coordinates that are not finite")
    if not s.is_cuda:
        return UVAtlasTable(s, Hu, Wu)
    n = s.shape[0] * s.shape[1] * s.shape[2]
    taps = torch.empty((n, 4), dtype=torch.int32, device=s.device)
    _lib.call("acfm_uv_atlas_taps", s.device, _lib.ptr(s), n, Hu, Wu, _lib.ptr(taps))
    return UVAtlasTable(s, Hu, Wu, *_uv_table_from_taps(taps, Hu * Wu))


class _UVAtlas(torch.autograd.Function):
    @staticmethod
    def forward(ctx, uvimage, table, nsym):
        x = uvimage.detach().contiguous()
        B = x.shape[0]
        atlas = torch.empty((B, table.Fp + nsym, table.T, table.T, 3), dtype=torch.float32, device=x.device)
        _lib.call("acfm_uv_atlas_forward", x.device, _lib.ptr(x), _lib.ptr(table.sampler), B, table.Hu, table.Wu,
                  table.Fp, table.T, nsym, _lib.ptr(atlas))
        ctx.save_for_backward(atlas)
        ctx.cfg = (table, nsym)
        return atlas

    @staticmethod
    def backward(ctx, go):
        atlas, = ctx.saved_tensors
        table, nsym = ctx.cfg
        g = _f32c(go)
        B = atlas.shape[0]
        gx = torch.empty((B, 3, table.Hu, table.Wu), dtype=torch.float32, device=atlas.device)
        _lib.call("acfm_uv_atlas_backward", atlas.device, _lib.ptr(g), _lib.ptr(atlas), _lib.ptr(table.sampler),
                  _lib.ptr(table.pix_start), _lib.ptr(table.pix_taps), table.n_entries, B, table.Hu, table.Wu, table.Fp,
                  table.T, nsym, _lib.ptr(gx))
        return gx, None, None


def uv_atlas(uvimage, table, num_sym_faces=0):
    """The tail of TexturePredictorUV.forward (mesh_net.py:169-179): uvimage [B,3,Hu,Wu] float32 -> atlas
    [B,F'+S,T,T,3] = (tanh(grid_sample(uvimage, sampler, align_corners=True)) + 1) / 2 per texel, the last S =
    num_sym_faces faces of the sampler once more behind the F'.  One launch forward, one backward (a gather per UV pixel
    over the table's lists: no atomics, bit-reproducible); nothing is allocated but the outputs, so both can be
    captured.  Host tensors run the reference's lines themselves."""
    if not isinstance(table, UVAtlasTable):
        raise ValueError("table: a UVAtlasTable (ops.uv_atlas_table(uv_sampler, Hu, Wu)) expected, got %s"
                         % type(table).__name__)
    if uvimage.dim() != 4 or uvimage.shape[1] != 3 or uvimage.shape[0] < 1:
        raise ValueError("uvimage: [B,3,Hu,Wu] expected (3 channels), got %s" % (tuple(uvimage.shape),))
    if uvimage.dtype != torch.float32:
        raise ValueError("uvimage must be float32, got %s" % uvimage.dtype)
    if tuple(uvimage.shape[2:]) != (table.Hu, table.Wu):
        raise ValueError("uvimage is %d x %d, the table was built for %d x %d"
                         % (uvimage.shape[2], uvimage.shape[3], table.Hu, table.Wu))
    nsym = int(num_sym_faces)
    if not 0 <= nsym <= table.Fp:
        raise ValueError("num_sym_faces must lie in [0, F'] = [0, %d], got %d" % (table.Fp, nsym))
    if uvimage.device != table.device:
        raise ValueError("uvimage is on %s, the table on %s" % (uvimage.device, table.device))
    if not uvimage.is_cuda:
        F_, T = table.Fp, table.T
        grid = table.sampler.view(1, F_, T * T, 2)
        tex = torch.nn.functional.grid_sample(uvimage, grid.repeat(uvimage.shape[0], 1, 1, 1), align_corners=True)
        tex = tex.reshape(uvimage.size(0), -1, F_, T, T).permute(0, 2, 3, 4, 1)
        tex = (torch.tanh(tex) + 1) / 2
        return torch.cat([tex, tex[:, F_ - nsym:]], 1) if nsym else tex
    return _UVAtlas.apply(uvimage, table, nsym)


# ------------------------------------------------------------------------------ perceptual texture loss (csrc/acfm_lpips.hip)
LPIPS_SHIFT = (-.030, -.088, -.188)     # lpips.ScalingLayer
LPIPS_SCALE = (.458, .448, .450)
LPIPS_EPS = 1e-10                       # lpips.normalize_tensor


def _lpips_batches(n_pred, ref, what):
    """(N, Nr) of a prediction batch against references given per prediction or once per frame (_ref_batch)."""
    return n_pred, _ref_batch(n_pred, ref, what)


class _LpipsInput(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, mask):
        i, m = _f32c(img), _f32c(mask)
        N, _, H, W = i.shape
        x = torch.empty_like(i)
        _lib.call("acfm_lpips_input_forward", i.device, _lib.ptr(i), _lib.ptr(m), N, m.shape[0], H, W, _lib.ptr(x))
        ctx.save_for_backward(m)
        return x

    @staticmethod
    def backward(ctx, gx):
        m, = ctx.saved_tensors
        g = _f32c(gx)
        N, _, H, W = g.shape
        gi = torch.empty_like(g)
        _lib.call("acfm_lpips_input_backward", g.device, _lib.ptr(g), _lib.ptr(m), N, m.shape[0], H, W, _lib.ptr(gi))
        return gi, None


def lpips_input(img, mask):
    """Step 1 of the perceptual loss in one pass: img [N,3,H,W], mask [N or N/G,H,W] (the ground-truth mask, shared by
    the G hypotheses of a frame) -> ((2 (img mask) - 1) - shift_c) / scale_c, the network's input.  Gradient to img
    only.  On the GPU img is not read where mask == 0 (a NaN there gives a NaN in the torch chain and none here).
    Host tensors run the torch chain itself."""
    if img.dim() != 4 or img.shape[1] != 3 or mask.dim() != 3 or tuple(mask.shape[1:]) != tuple(img.shape[2:]):
        raise ValueError("lpips_input: img [N,3,H,W] and mask [N or N/G,H,W] expected, got %s and %s"
                         % (tuple(img.shape), tuple(mask.shape)))
    N, Nr = _lpips_batches(img.shape[0], mask, "lpips_input")
    if img.device != mask.device:
        raise ValueError("lpips_input: img is on %s, mask on %s" % (img.device, mask.device))
    if not img.is_cuda:
        m = mask.to(img.dtype).repeat(N // Nr, 1, 1).unsqueeze(1)
        x = 2 * (img * m) - 1
        return (x - x.new_tensor(LPIPS_SHIFT)[None, :, None, None]) / x.new_tensor(LPIPS_SCALE)[None, :, None, None]
    return _LpipsInput.apply(img, mask.detach())


def _ptr_at(t, offset):
    return ctypes.c_void_p(t.data_ptr() + 4 * int(offset))


class _LpipsLayers(torch.autograd.Function):
    """d [N,P]: the layers' distance maps side by side.  args = fa_0.., fb_0.., lin_0.. (L of each; lin may be None)."""
    @staticmethod
    def forward(ctx, L, *args):
        fas = [_f32c(t) for t in args[:L]]
        fbs = [_f32c(t) for t in args[L:2 * L]]
        lins = [None if t is None else _f32c(t) for t in args[2 * L:]]
        N, Nr = fas[0].shape[0], fbs[0].shape[0]
        hws = [int(t[0, 0].numel()) for t in fas]
        P = sum(hws)
        d = torch.empty((N, P), dtype=torch.float32, device=fas[0].device)
        off = 0
        for a, b, w, hw in zip(fas, fbs, lins, hws):
            _lib.call("acfm_lpips_layer_forward", a.device, _lib.ptr(a), _lib.ptr(b), _lib.ptr(w), N, Nr, a.shape[1], hw,
                      _ptr_at(d, off), P)
            off += hw
        ctx.save_for_backward(*fas, *fbs, *[w for w in lins if w is not None])
        ctx.cfg = (L, [w is not None for w in lins], hws, P)
        return d

    @staticmethod
    def backward(ctx, gd):
        L, has_lin, hws, P = ctx.cfg
        saved = list(ctx.saved_tensors)
        fas, fbs, rest = saved[:L], saved[L:2 * L], saved[2 * L:]
        lins = [rest.pop(0) if h else None for h in has_lin]
        g = _f32c(gd)
        N, Nr = fas[0].shape[0], fbs[0].shape[0]
        need_a, need_b = ctx.needs_input_grad[1:1 + L], ctx.needs_input_grad[1 + L:1 + 2 * L]
        ga, gb = [None] * L, [None] * L
        off = 0
        for l, (a, b, w, hw) in enumerate(zip(fas, fbs, lins, hws)):
            if need_a[l]:
                ga[l] = torch.empty_like(a)
                _lib.call("acfm_lpips_layer_backward", a.device, _lib.ptr(a), _lib.ptr(b), _lib.ptr(w), _ptr_at(g, off), P,
                          N, Nr, a.shape[1], hw, _lib.ptr(ga[l]))
            if need_b[l]:   # Nr == N (checked by lpips_layers): d is symmetric, the same kernel with the roles exchanged
                gb[l] = torch.empty_like(b)
                _lib.call("acfm_lpips_layer_backward", a.device, _lib.ptr(b), _lib.ptr(a), _lib.ptr(w), _ptr_at(g, off), P,
                          N, N, a.shape[1], hw, _lib.ptr(gb[l]))
            off += hw
        return (None, *ga, *gb, *([None] * L))


def _lpips_layer_host(fa, fb, lin):
    """The definition from torch ops: u = a / (|a| + eps), v likewise, d = sum_c lin_c (u - v)^2 -> [N,hw]; at an
    all-zero vector u = 0 and the norm sends no gradient."""
    N, Nr = fa.shape[0], fb.shape[0]

    def unit(x):
        s = (x * x).sum(1, keepdim=True)
        pos = s > 0
        n = torch.where(pos, torch.sqrt(torch.where(pos, s, torch.ones_like(s))), torch.zeros_like(s))
        return x / (n + LPIPS_EPS)
    diff = (unit(fa) - unit(fb).repeat(N // Nr, 1, 1, 1)) ** 2
    if lin is not None:
        diff = diff * lin.reshape(1, -1, 1, 1)
    return diff.sum(1).reshape(N, -1)


def lpips_layers(fas, fbs, lins=None):
    """Step 3 of the perceptual loss for a list of layers: fas[l] [N,C_l,h_l,w_l] (prediction features, after the
    ReLU), fbs[l] [N or N/G,C_l,h_l,w_l] (reference features), lins[l] [C_l] non-negative weights or None (= 1, the
    reference's lpips=False) -> d [N,P], P = sum h_l w_l, the layers' maps side by side:
        d = sum_c lin_c (a_c / (|a| + 1e-10) - b_c / (|b| + 1e-10))^2   per pixel.
    One launch per layer each way; gradients to fas, and to fbs when they have the predictions' batch (a reference
    shared by G predictions that requires grad is refused).  At a pixel whose feature vector is all zero u = 0 and the
    norm's gradient term is dropped (lpips's autograd gives NaN there).  Host tensors run the same definition from
    torch ops."""
    fas, fbs = list(fas), list(fbs)
    L = len(fas)
    lins = [None] * L if lins is None else list(lins)
    if L < 1 or len(fbs) != L or len(lins) != L:
        raise ValueError("lpips_layers: as many reference maps and weight vectors as prediction maps expected")
    N, Nr = _lpips_batches(fas[0].shape[0], fbs[0], "lpips_layer")
    for a, b, w in zip(fas, fbs, lins):
        if a.dim() != 4 or b.dim() != 4 or a.shape[1:] != b.shape[1:] or a.shape[0] != N or b.shape[0] != Nr \
                or a[0].numel() == 0:
            raise ValueError("lpips_layer: fa [N,C,h,w] and fb [N or N/G,C,h,w] expected, got %s and %s"
                             % (tuple(a.shape), tuple(b.shape)))
        if a.dtype != torch.float32 or b.dtype != torch.float32:
            raise ValueError("lpips_layer: float32 features expected, got %s and %s" % (a.dtype, b.dtype))
        if w is not None and (w.numel() != a.shape[1] or w.requires_grad):
            raise ValueError("lpips_layer: lin must hold one constant weight per channel (%d), got %s"
                             % (a.shape[1], tuple(w.shape)))
        if b.requires_grad and Nr != N and torch.is_grad_enabled():
            raise ValueError("lpips_layer: a reference shared by %d predictions each (batch %d for %d) cannot require "
                             "grad; repeat it to the predictions' batch" % (N // Nr, Nr, N))
        if a.device != b.device or (w is not None and w.device != a.device):
            raise ValueError("lpips_layer: features and weights must be on one device")
    if not fas[0].is_cuda:
        return torch.cat([_lpips_layer_host(a, b, w) for a, b, w in zip(fas, fbs, lins)], 1)
    return _LpipsLayers.apply(L, *fas, *fbs, *[None if w is None else w.detach().reshape(-1) for w in lins])


def lpips_layer(fa, fb, lin=None):
    """One layer of lpips_layers: fa [N,C,h,w], fb [N or N/G,C,h,w], lin [C] or None -> d [N,h,w]."""
    return lpips_layers([fa], [fb], [lin]).reshape(fa.shape[0], fa.shape[2], fa.shape[3])


def lpips_mask_weights(mask, sizes):
    """M [Nr,P] for mask [Nr,H,W] and the layers' sizes [(h_l, w_l), ...]: M_l = U_l^T (mask / (H W)), U_l the bilinear
    upsampling (h_l,w_l) -> (H,W) with align_corners=False.  Upsampling is linear, so
        mean_{H,W}(mask * sum_l upsample(d_l)) = sum_p d[p] M[p]
    and the loss needs neither the upsampled maps nor their sum (lpips_masked_mean).  M depends on the ground-truth
    mask only: no gradient.  One launch, bit-reproducible.  Host tensors take the adjoint from autograd."""
    sizes = [(int(h), int(w)) for h, w in sizes]
    if mask.dim() != 3 or mask.shape[0] < 1 or mask[0].numel() == 0:
        raise ValueError("lpips_mask_weights: mask [Nr,H,W] expected, got %s" % (tuple(mask.shape),))
    if not 1 <= len(sizes) <= 8 or any(h < 1 or w < 1 for h, w in sizes):
        raise ValueError("lpips_mask_weights: 1 to 8 layer sizes (h, w) >= 1 expected, got %s" % (sizes,))
    Nr, H, W = mask.shape
    if not mask.is_cuda:
        m = mask.detach().to(torch.float32)[:, None] / (H * W)
        out = []
        with torch.enable_grad():
            for h, w in sizes:
                z = torch.zeros((Nr, 1, h, w), dtype=torch.float32, requires_grad=True)
                up = torch.nn.functional.interpolate(z, size=(H, W), mode="bilinear", align_corners=False)
                out.append(torch.autograd.grad((up * m).sum(), z)[0].reshape(Nr, -1))
        return torch.cat(out, 1)
    m = _f32c(mask.detach())
    P = sum(h * w for h, w in sizes)
    M = torch.empty((Nr, P), dtype=torch.float32, device=m.device)
    hw = (ctypes.c_int32 * (2 * len(sizes)))(*[v for s in sizes for v in s])
    _lib.call("acfm_lpips_mask_weights", m.device, _lib.ptr(m), Nr, H, W, hw, len(sizes), _lib.ptr(M))
    return M


class _LpipsMaskedMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, d, M):
        dd, mm = _f32c(d), _f32c(M)
        N, P = dd.shape
        loss = torch.empty((N,), dtype=torch.float32, device=dd.device)
        _lib.call("acfm_lpips_masked_mean_forward", dd.device, _lib.ptr(dd), _lib.ptr(mm), N, mm.shape[0], P,
                  _lib.ptr(loss))
        ctx.save_for_backward(mm)
        return loss

    @staticmethod
    def backward(ctx, gl):
        mm, = ctx.saved_tensors
        g = _f32c(gl)
        N, P = g.shape[0], mm.shape[1]
        gd = torch.empty((N, P), dtype=torch.float32, device=g.device)
        _lib.call("acfm_lpips_masked_mean_backward", g.device, _lib.ptr(g), _lib.ptr(mm), N, mm.shape[0], P, _lib.ptr(gd))
        return gd, None


def lpips_masked_mean(d, M):
    """loss [N] = sum_p d[n,p] M[n % Nr,p] for d [N,P] (lpips_layers) and M [N or N/G,P] (lpips_mask_weights): the mean
    over the image of mask * (the upsampled layer maps' sum), without forming it.  Gradient to d only.  One workgroup
    per row in a fixed order (bit-reproducible); the output is written, never accumulated."""
    if d.dim() != 2 or M.dim() != 2 or d.shape[1] != M.shape[1] or d.shape[1] < 1:
        raise ValueError("lpips_masked_mean: d [N,P] and M [N or N/G,P] expected, got %s and %s"
                         % (tuple(d.shape), tuple(M.shape)))
    N, Nr = _lpips_batches(d.shape[0], M, "lpips_masked_mean")
    if d.device != M.device:
        raise ValueError("lpips_masked_mean: d is on %s, M on %s" % (d.device, M.device))
    if not d.is_cuda:
        return (d * M.detach().repeat(N // Nr, 1)).sum(1)
    return _LpipsMaskedMean.apply(d, M.detach())


# ------------------------------------------------------------------------------ keypoint supervision (csrc/acfm_keypoints.hip)
KP_MAX_K = 64          # keypoints: one lane each
KP_MAX_V = 65535
KP_MAX_N = 65535


def _kp_f32(name, *tensors):
    for t in tensors:
        if t is not None and t.dtype != torch.float32:
            raise ValueError("%s: float32 only, got %s" % (name, t.dtype))


def _kp_limits(name, K, V, N=0, Nv=1, Ng=1):
    if not 1 <= K <= KP_MAX_K:
        raise ValueError("%s: 1 <= K <= %d keypoints, got K = %d" % (name, KP_MAX_K, K))
    if not 1 <= V <= KP_MAX_V:
        raise ValueError("%s: 1 <= V <= %d vertices, got V = %d" % (name, KP_MAX_V, V))
    if N > KP_MAX_N:
        raise ValueError("%s: N <= %d cameras, got N = %d" % (name, KP_MAX_N, N))
    if N and (Nv < 1 or N % Nv):
        raise ValueError("%s: N %% Nv == 0: %d cameras do not share %d rows of vertices evenly" % (name, N, Nv))
    if N and (Ng < 1 or N % Ng):
        raise ValueError("%s: N %% Ng == 0: %d cameras do not share %d rows of ground truth evenly" % (name, N, Ng))


class _KpWeights(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits):
        ctx.set_materialize_grads(False)
        x = _f32c(logits)
        K, V = x.shape
        A = torch.empty_like(x)
        entropy = torch.empty((), dtype=torch.float32, device=x.device)
        stats = torch.empty((K, 2), dtype=torch.float32, device=x.device)
        _lib.call("acfm_kp_weights_forward", x.device, _lib.ptr(x), K, V, _lib.ptr(A), _lib.ptr(entropy), _lib.ptr(stats))
        ctx.save_for_backward(x, A, stats)
        return A, entropy

    @staticmethod
    def backward(ctx, gA, ge):
        if gA is None and ge is None:
            return None
        x, A, stats = ctx.saved_tensors
        K, V = x.shape
        gA = None if gA is None else _f32c(gA)
        ge = None if ge is None else _f32c(ge)
        gx = torch.empty_like(x)
        _lib.call("acfm_kp_weights_backward", x.device, _lib.ptr(x), _lib.ptr(A), _lib.ptr(stats), _lib.ptr(gA),
                  _lib.ptr(ge), K, V, _lib.ptr(gx))
        return gx


def kp_weights(logits):
    """vert2kp logits [K,V] -> (A = softmax(logits, 1) [K,V], entropy_loss(A) as a scalar) from one launch each way
    (mesh_net.py:504-519's softmax, loss_utils.py:330-338).  The entropy is evaluated from the log-softmax, so it and
    its gradient stay finite where A underflows to 0 (the reference's A * log(A) is NaN there)."""
    if logits.dim() != 2:
        raise ValueError("kp_weights: logits [K,V] expected, got %s" % (tuple(logits.shape),))
    _kp_f32("kp_weights", logits)
    _kp_limits("kp_weights", logits.shape[0], logits.shape[1])
    _lib.require_gpu(logits)
    return _KpWeights.apply(logits)


class _KpHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, A, verts, cams, kp_gt, img_size, want_err):
        ctx.set_materialize_grads(False)
        a, v, c = _f32c(A), _f32c(verts), _f32c(cams)
        g = None if kp_gt is None else _f32c(kp_gt)
        K, V = a.shape
        Nv, N, Ng = v.shape[0], c.shape[0], (1 if g is None else g.shape[0])
        dev = a.device
        kp_verts = torch.empty((Nv, K, 3), dtype=torch.float32, device=dev)
        kp_pred = torch.empty((N, K, 2), dtype=torch.float32, device=dev)
        loss = None if g is None else torch.empty((N,), dtype=torch.float32, device=dev)
        err = torch.empty((N, K), dtype=torch.float32, device=dev) if want_err else None
        _lib.call("acfm_kp_head_forward", dev, _lib.ptr(a), _lib.ptr(v), _lib.ptr(c), _lib.ptr(g), K, V, N, Nv, Ng,
                  float(img_size or 0.0), _lib.ptr(kp_verts), _lib.ptr(kp_pred), _lib.ptr(loss), _lib.ptr(err))
        ctx.save_for_backward(a, v, c, g, kp_verts, kp_pred)
        if err is not None:
            ctx.mark_non_differentiable(err)
        return kp_verts, kp_pred, loss, err

    @staticmethod
    def backward(ctx, g_kpv, g_pred, g_loss, _g_err):
        a, v, c, gt, kp_verts, kp_pred = ctx.saved_tensors
        need = ctx.needs_input_grad
        if not any(need[:3]) or (g_kpv is None and g_pred is None and g_loss is None):
            return None, None, None, None, None, None
        K, V = a.shape
        Nv, N, Ng = v.shape[0], c.shape[0], (1 if gt is None else gt.shape[0])
        dev = a.device
        g_kpv, g_pred, g_loss = [None if t is None else _f32c(t) for t in (g_kpv, g_pred, g_loss)]
        gA = torch.empty_like(a) if need[0] else None
        gv = torch.empty_like(v) if need[1] else None
        gc = torch.empty_like(c) if need[2] else None
        nb = int(_lib.lib().acfm_kp_head_workspace_bytes(K, Nv))
        ws = torch.empty((nb,), dtype=torch.uint8, device=dev)
        _lib.call("acfm_kp_head_backward", dev, _lib.ptr(a), _lib.ptr(v), _lib.ptr(c), _lib.ptr(gt), _lib.ptr(kp_verts),
                  _lib.ptr(kp_pred), _lib.ptr(g_loss), _lib.ptr(g_pred), _lib.ptr(g_kpv), K, V, N, Nv, Ng, _lib.ptr(gA),
                  _lib.ptr(gv), _lib.ptr(gc), _lib.ptr(ws), nb)
        return gA, gv, gc, None, None, None


def kp_head(A, verts, cams, kp_gt=None, img_size=None, want_err=False):
    """The keypoint head in one launch (two or three back): A [K,V] (kp_weights), verts [Nv,V,3], cams [N,7],
    kp_gt [Ng,K,3] (x, y, visibility) or None -> (kp_verts [Nv,K,3] = A @ verts, kp_pred [N,K,2] = its projection --
    the bits of project_xy(kp_verts, cams) --, loss [N] = kp_l2_loss(kp_pred, kp_gt, reduction='none') or None,
    kp_err [N,K] = evaluate.py:156-158's pixel error (want_err=True, needs img_size; no gradient) or None).
    Camera n reads vertices n % Nv and ground truth n % Ng: the G hypotheses of a frame share both, as the reference's
    repeat(G, 1, 1) copies would.  Gradients to A, verts and cams; d|x| at 0 is 0."""
    if A.dim() != 2 or verts.dim() != 3 or verts.shape[2] != 3 or verts.shape[1] != A.shape[1] \
            or cams.dim() != 2 or cams.shape[1] != 7:
        raise ValueError("kp_head: A [K,V], verts [Nv,V,3], cams [N,7] expected, got %s, %s, %s"
                         % (tuple(A.shape), tuple(verts.shape), tuple(cams.shape)))
    K, V = A.shape
    if kp_gt is not None and (kp_gt.dim() != 3 or kp_gt.shape[1] != K or kp_gt.shape[2] != 3):
        raise ValueError("kp_head: kp_gt [Ng,%d,3] expected, got %s" % (K, tuple(kp_gt.shape)))
    if want_err and (kp_gt is None or img_size is None):
        raise ValueError("kp_head: want_err needs kp_gt and img_size")
    if cams.shape[0] == 0:          # (the library launches nothing for N == 0, kp_verts included)
        raise ValueError("kp_head: at least one camera, got cams %s" % (tuple(cams.shape),))
    _kp_f32("kp_head", A, verts, cams, kp_gt)
    _kp_limits("kp_head", K, V, cams.shape[0], verts.shape[0], 1 if kp_gt is None else kp_gt.shape[0])
    _lib.require_gpu(A, verts, cams, kp_gt)
    return _KpHead.apply(A, verts, cams, None if kp_gt is None else kp_gt.detach(), img_size, bool(want_err))


class _CameraLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cam_pred, cam_ref, cams, probs, margin):
        ctx.set_materialize_grads(False)
        p = _f32c(cam_pred)
        r, c, w = [None if t is None else _f32c(t) for t in (cam_ref, cams, probs)]
        N, dev = p.shape[0], p.device
        G = 0 if w is None else w.shape[0]
        loss = torch.empty((), dtype=torch.float32, device=dev)
        best = None if w is None else torch.empty((N,), dtype=torch.int64, device=dev)
        _lib.call("acfm_camera_loss_forward", dev, _lib.ptr(p), _lib.ptr(r), _lib.ptr(c), _lib.ptr(w), N, G,
                  float(margin), _lib.ptr(loss), _lib.ptr(best))
        ctx.save_for_backward(p, r, c, best)
        ctx.margin = float(margin)
        if best is not None:
            ctx.mark_non_differentiable(best)
        return loss, best

    @staticmethod
    def backward(ctx, g, _gb):
        if g is None or not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        p, r, c, best = ctx.saved_tensors
        g = _f32c(g)
        gp = torch.empty_like(p)
        _lib.call("acfm_camera_loss_backward", p.device, _lib.ptr(p), _lib.ptr(r), _lib.ptr(c), _lib.ptr(best),
                  _lib.ptr(g), p.shape[0], ctx.margin, _lib.ptr(gp))
        return gp, None, None, None, None


def camera_loss(cam_pred, cam_ref=None, margin=0., cams=None, probs=None):
    """loss_utils.camera_loss(cam_pred, cam_ref, margin) in one launch each way -> (loss, None); or, with cams [G*N,7]
    and probs [G,N] in place of cam_ref, against the most probable hypothesis of every frame (multiframe/main.py:753-762:
    argmax, gather, detach, camera_loss) -> (loss, best [N] int64 = probs.argmax(0), the smallest g at a tie).
    Only cam_pred receives a gradient."""
    if (cam_ref is None) == (cams is None) or (cams is None) != (probs is None):
        raise ValueError("camera_loss: give either cam_ref [N,7] or cams [G*N,7] with probs [G,N]")
    if cam_pred.dim() != 2 or cam_pred.shape[1] != 7:
        raise ValueError("camera_loss: cam_pred [N,7] expected, got %s" % (tuple(cam_pred.shape),))
    N = cam_pred.shape[0]
    if cam_ref is not None and tuple(cam_ref.shape) != (N, 7):
        raise ValueError("camera_loss: cam_ref [%d,7] expected, got %s" % (N, tuple(cam_ref.shape)))
    if cams is not None and (probs.dim() != 2 or probs.shape[1] != N or probs.shape[0] < 1
                             or tuple(cams.shape) != (probs.shape[0] * N, 7)):
        raise ValueError("camera_loss: cams [G*%d,7] and probs [G,%d] expected, got %s and %s"
                         % (N, N, tuple(cams.shape), tuple(probs.shape)))
    if N > KP_MAX_N:
        raise ValueError("camera_loss: N <= %d cameras, got N = %d" % (KP_MAX_N, N))
    _kp_f32("camera_loss", cam_pred, cam_ref, cams, probs)
    _lib.require_gpu(cam_pred, cam_ref, cams, probs)
    det = lambda t: None if t is None else t.detach()
    return _CameraLoss.apply(cam_pred, det(cam_ref), det(cams), det(probs), margin)
