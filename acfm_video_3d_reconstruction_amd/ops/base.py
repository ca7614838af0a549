"""What every operator family uses: tensor coercion, LazyGrad, the face-list memo, workspaces, the capture id, reference
batches and the ticket / partial-sum scratch.  Depends on nothing else in the package."""
import ctypes
import threading

import torch

from .. import _lib


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


def _f32c(t):
    if type(t) is LazyGrad:          # a gradient another operator of this package has not formed yet
        t = t.materialize()
    return t.detach().to(torch.float32).contiguous()


def _real(t, f16):
    """Storage tensor of the raster ops: float32, or float16 with storage="f16" (ACFM_STORE_F16)."""
    return t.detach().to(torch.float16 if f16 else torch.float32).contiguous()


def _is_f16(storage):
    if storage not in ("f32", "f16"):
        raise ValueError("storage must be 'f32' or 'f16', got %r" % (storage,))
    return storage == "f16"


# The caches of the package (_FACES and the loss scratch here, _SETUP and _COVER in render.py) are shared by the threads
# nn.DataParallel runs its replicas on (main.py:183-193): every read-modify-write of them happens under _LOCK.
_LOCK = threading.RLock()
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


def _capture_id(device):
    """0 when the current stream of `device` is not capturing, else the id of the capture."""
    if not torch.cuda.is_current_stream_capturing():
        return 0
    cid = ctypes.c_ulonglong(0)
    _lib.check(_lib.lib().acfm_stream_capture_id(_lib.cur_stream(device), ctypes.byref(cid)), "acfm_stream_capture_id")
    return int(cid.value) or -1


def _ref_batch(N, ref, what):
    """References (ground-truth masks, images, boundary points) may be given once per frame for the G
    hypotheses rendered of it: [N/G, ...] against N predictions, prediction n <-> reference n % (N/G)
    (= the trainer's ref.repeat(G, ...) without the copies)."""
    RB = ref.shape[0]
    if RB <= 0 or N % RB != 0:
        raise ValueError("%s: %d references for %d predictions (must divide)" % (what, RB, N))
    return RB


def _i64c(t):
    return t.detach().to(torch.int64).contiguous()


def _a16(t):
    """float32 contiguous, 16-byte aligned (the RGBA planes are read as float4)."""
    t = _f32c(t)
    return t if t.data_ptr() % 16 == 0 else t.clone()


# Scratch of the one-launch loss sums (acfm_mask_losses, acfm_tex_mse, acfm_bds_loss given tickets: include/acfm_hip.h):
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
    """-> (tickets, partials, floats in partials) for a ticket-form call of loss `which` on the current stream."""
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
