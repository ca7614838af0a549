"""The renders and the caches they share: silhouette, hard raster, atlas texture and vertex colour, the face-setup /
cover / prefill hand-over between them, LazyPixToFace."""
import dataclasses
import math

import torch

from .. import _lib
from .base import LazyGrad, _LOCK, _capture_id, _f32c, _is_f16, _real, _ref_batch, _workspace, expand_faces
from .pending import flush_pending_losses

SIL_K = 20  # nmr.py:158
SIL_SIGMA = 1e-4  # nmr.py:153
SIL_BLUR = math.log(1.0 / 1e-4 - 1.0) * 1e-4  # nmr.py:157


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
# The caches below (_SETUP, _COVER) and base._FACES are shared by the threads nn.DataParallel runs its replicas on
# (main.py:183-193): every read-modify-write of them happens under base._LOCK.
_SETUP = {}
_EPOCH = [0]
_SHARE = [True]


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


def _setup_key(v, c, f, H, offset_z):
    return (v.data_ptr(), v._version, tuple(v.shape), c.data_ptr(), c._version, f.data_ptr(), f._version,
            tuple(f.shape), int(H), float(offset_z), torch.cuda.current_stream(v.device).cuda_stream,
            _capture_id(v.device), _EPOCH[0])


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
        _lib.call("acfm_sil_forward", v.device, v, f, c, N, V, F, H, K, K, float(blur), float(sigma), float(offset_z),
                  mask, full, kth, vis2, ws, nb, _lib.tuning_ptr(tune), None)
        return full

    return LazyPixToFace(plane0, K, make_full, vis)


# ------------------------------------------------------------------------------ silhouette
class _SilRender(torch.autograd.Function):
    """Soft silhouette render (acfm_sil_forward / acfm_sil_backward); fused=True: the render and its [N,4]
    silhouette-loss vector against gt / edt as one operator (acfm_sil_loss_forward / acfm_sil_loss_backward),
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
        if fused:
            _lib.call("acfm_sil_loss_forward", v.device, v, f, c, g, e, RB, N, V, F, H, K, int(k_out), float(blur),
                      float(sigma), float(offset_z), mask, p2f, kth, vis, losses, ws, nb, tp, exp)
        else:
            _lib.call("acfm_sil_forward", v.device, v, f, c, N, V, F, H, K, int(k_out), float(blur), float(sigma),
                      float(offset_z), mask, p2f, kth, vis, ws, nb, tp, exp)
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
        if glosses is None and gmask is None:      # only the projection was used: its own backward
            _lib.call("acfm_project_xy_backward", v.device, v, c, gp, N, V, gv, gc)
            return (gv, None, gc) + none[3:]
        ws, nb, tune = ctx.ws
        exp, _ex_keep = _lib.sil_extras(grad_proj_xy=gp)
        if glosses is not None:       # the fused operator
            pay = (mask, g, e, RB, _f32c(glosses))
        else:                         # the silhouette losses' gradient, still unformed: the kernel forms it per pixel
            pay = gmask.take("mask_losses", mask) if type(gmask) is LazyGrad else None
        if pay is not None:
            _m, lg, le, rb, go = pay
            _lib.call("acfm_sil_loss_backward", v.device, v, f, c, mask, kth, lg, le, rb, go, N, V, F, H, blur, sigma,
                      offset_z, gv, gc, ws, nb, 1, _lib.tuning_ptr(tune), exp)
        else:
            gm = _f32c(gmask)
            _lib.call("acfm_sil_backward", v.device, v, f, c, mask, kth, gm, N, V, F, H, blur, sigma, offset_z, gv, gc,
                      ws, nb, 1, _lib.tuning_ptr(tune), exp)
        return (gv, None, gc) + none[3:]


def _proj_key(verts, cams):
    """What a projection handed from a silhouette render to NeuralRenderer.project_points must share with the call it
    answers: the storage (address, version, shape, dtype) AND the autograd identity the result would have -- which
    input requires grad, whether the graph is being recorded -- and the hipGraph capture (a tensor made inside a capture
    lives in the graph's pool and is rewritten by every replay: it serves that capture only)."""
    return (verts.data_ptr(), verts._version, tuple(verts.shape), str(verts.dtype), cams.data_ptr(), cams._version,
            tuple(cams.shape), str(cams.dtype), bool(verts.requires_grad), bool(cams.requires_grad),
            torch.is_grad_enabled(), _capture_id(verts.device) if verts.is_cuda else 0)


def _proj_serves(entry, verts, cams):
    """entry = (key, proj, (verts, cams) of the render: kept alive, so that the addresses in the key cannot be
    recycled -- like _Setup.inputs).  True when `proj` is what project_xy(verts, cams) would return, gradient path
    included: the key matches, and an input the graph was recorded for is the render's very tensor object (`v.detach()`
    and a new leaf on the same storage share address and version with `v`, but not its place in the graph)."""
    key, _proj, inputs = entry
    if key != _proj_key(verts, cams):
        return False
    recorded = torch.is_grad_enabled()
    return all(a is b or not (recorded and b.requires_grad) for a, b in zip(inputs, (verts, cams)))


def _sil_apply(verts, faces, cams, gt, edt, img_size, K, blur, sigma, offset_z, k_out, storage, fused):
    """_SilRender with the k_out / lazy resolution of both wrappers; -> (losses or None, mask, pix_to_face)."""
    f16 = _is_f16(storage)
    lazy = k_out == "lazy" and not f16 and K > 1
    # (half storage: the default is the one plane it can write; a k_out the caller NAMES reaches the operator's check)
    unnamed = k_out in (None, "lazy")
    losses, mask, p2f, vis, proj = _SilRender.apply(verts, faces, cams, gt, edt, img_size, K, blur, sigma, offset_z,
                                                    1 if (lazy or (f16 and unnamed)) else (K if unnamed else int(k_out)),
                                                    f16, fused)
    if lazy:   # k_out="lazy": [N,H,H,K] whose slots 1.. are rendered on first use (LazyPixToFace)
        p2f = _lazy_pix_to_face(p2f, vis, _f32c(verts), expand_faces(faces, verts.shape[0]), _f32c(cams),
                                int(img_size), int(K), blur, sigma, offset_z)
    else:
        p2f._acfm_vis = vis
    # the (x, y) projection of these vertices under these cameras, an output of the render's autograd node: rides on
    # the pix_to_face object like the visibility bitmap (NeuralRenderer.project_points picks it up)
    p2f._acfm_proj = (_proj_key(verts, cams), proj, (verts, cams))
    return losses, mask, p2f


def sil_render(verts, faces, cams, img_size, K=SIL_K, blur=SIL_BLUR, sigma=SIL_SIGMA, offset_z=0.0,
               k_out=None, storage="f32"):
    """Soft silhouette: -> (mask [N,H,H] f32, pix_to_face [N,H,H,k_out] i64), k_out = K (default,
    what PyTorch3D returns) or 1 (nearest-face plane only; K faces are still blended).
    The visible-vertex bitmap the raster kernel produces on the side (vertices of every
    nearest face, = what bds_loss / optical_flow_loss derive from pix_to_face[..., 0]) rides
    along on the pix_to_face tensor object as `._acfm_vis`.
    storage="f16": mask [N,H,H] float16, pix_to_face [N,H,H,1] int32 (BASELINE config 5); fp32 arithmetic.  That
    plane is the default there; any other k_out given by number raises ValueError."""
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
    _lib.call("acfm_hard_raster", v.device, v, f, N, V, F, H, p2f, vis, ws, nb, _lib.tuning()[0])
    p2f._acfm_vis = vis
    return p2f


# ------------------------------------------------------------------------------ texture
# atlas gradient: gather per face over the pixels of its box (acfm_tex_backward_faces, R <= 8) instead
# of one global float atomic per pixel and channel (acfm_tex_backward); both are kept and tested
TEX_BWD_GATHER = [True]


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
        if fused:
            _lib.call("acfm_tex_mse_forward", v.device, v, f, c, a, ri, rm, RB, N, V, F, H, R, float(sigma),
                      float(gamma), float(offset_z), imgs, sil, p2f, tidx, loss, ws, nb, ws_ready, float(ws_blur), NA,
                      _lib.tuning_ptr(tune))
        else:
            _lib.call("acfm_tex_forward", v.device, v, f, c, a, N, V, F, H, R, float(sigma), float(gamma),
                      float(offset_z), imgs, sil, p2f, tidx, ws, nb, ws_ready, float(ws_blur), NA,
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
        elif type(gimgs) is LazyGrad and TEX_BWD_GATHER[0] and R <= 8 and not ctx.f16:
            pay = gimgs.take("tex_mse", imgs)
        else:
            pay = None
        ws, nb, ws_blur = ctx.ws
        ga = None
        if pay is not None:      # the texture MSE's gradient (a LazyGrad still unformed): the kernel forms it per pixel
            t0, ri, rm, rb, go = pay
            ga = torch.empty((NA, F, R, R, 3), dtype=torch.float32, device=t0.device)
            _lib.call("acfm_tex_mse_backward_faces", t0.device, t0, ri, rm, rb, go, tidx, ws, nb, ws_blur, N, V, F, H,
                      R, NA, ga, _lib.tuning_ptr(ctx.tune))
        elif gimgs is not None:
            g = _f32c(gimgs)
            ga = torch.empty((NA, F, R, R, 3), dtype=torch.float32, device=g.device)
            if TEX_BWD_GATHER[0] and R <= 8:
                _lib.call("acfm_tex_backward_faces", g.device, g, tidx, ws, nb, ws_blur, N, V, F, H, R, NA, ga)
            else:
                _lib.call("acfm_tex_backward", g.device, g, tidx, N, F, H, R, NA, ga)
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
    _lib.call("acfm_vertex_color_forward", v.device, v, f, c, col, N, V, F, H, float(sigma), float(gamma),
              float(offset_z), imgs, sil, p2f, ws, nb, 0, 0.0, _lib.tuning()[0])
    return imgs, sil, p2f


# ------------------------------------------------------------------------------ visible vertices
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
    _lib.call("acfm_visible_vertices", p.device, p, f, N, nv, f.shape[1], HW, K, vis)
    return vis
