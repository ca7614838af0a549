"""Deferred loss terms: PendingTerm, its jobs and the one-launch step tail (acfm_step_losses_forward)."""
import contextlib
import ctypes
import threading
import weakref

import torch

from .. import _lib
from .base import _LOCK, _capture_id, _row_scratch


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
# the cover flag of render.py follows what the texture renders do); a term that a capture returns unread is launched where
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
                  ref(structs.get("bds")), ref(tot), N, tk, part, nf)
    finally:
        for j in jobs:
            j.taken(fused=True)
