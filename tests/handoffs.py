"""Helpers of the hand-off tests (test_gpu_handoff_*.py, test_handoff_memos.py): the layer that decides which kernel runs
and whose result is handed to whom -- shortcuts keyed on tensor identity (address, version, shape) or kept as module
state.  No tests in here.

    dropping(t); del t; new = recycled(make)     a new tensor ON THE ADDRESS of one that has just been dropped
    with plain(lazy=True, share=True): ...       the same calls with the shortcut switched off
    grads(loss, leaves)                          gradients with a missing path as zeros
    scene(...), solver_case(...)                 the inputs every case uses"""
import contextlib

import numpy as np
import pytest
import torch

from helpers import batch_verts, fps_lbs_logits, make_cams

_DROPPED = []


def dropping(t):
    """Note the address of a tensor the caller is about to drop (`dropping(t); del t`) for recycled()."""
    _DROPPED[:] = [(t.data_ptr(), t.device)]


def recycled(make, attempts=4):
    """make() -> a fresh tensor; called until the tensor lands on the address noted by dropping().  The caching
    allocator hands a just-freed block to an equal-sized request on the same stream, so one attempt is the norm.  If
    the address never comes back the test shows nothing about recycling: it FAILS (no skip, no silent pass)."""
    ptr, device = _DROPPED[0]
    if device.type == "cuda":
        torch.cuda.synchronize(device)
    others = []                      # (kept until the end: a block we hold cannot be handed out again)
    for _ in range(attempts):
        t = make()
        if t.data_ptr() == ptr:
            return t
        others.append(t)
    pytest.fail("address was not reused: this test shows nothing")


def pinned(make, attempts=4):
    """The other half: while something under test rightly HOLDS the block noted by dropping(), no new tensor may land
    on it.  make() is called `attempts` times, every tensor kept; -> the tensors, after asserting that none of them
    has the noted address."""
    ptr, device = _DROPPED[0]
    if device.type == "cuda":
        torch.cuda.synchronize(device)
    made = [make() for _ in range(attempts)]
    assert all(t.data_ptr() != ptr for t in made), "the block was handed out again while an entry should hold it"
    return made


@contextlib.contextmanager
def plain(lazy=False, share=False):
    """Turn shortcuts off where a switch exists and restore them whatever happens: lazy -> ops.LAZY_GRADS (unformed image
    gradients), share -> ops.share_setup (silhouette -> texture workspace take-over)."""
    from acfm_video_3d_reconstruction_amd import ops
    old_lazy, old_share = ops.LAZY_GRADS[0], None
    try:
        if lazy:
            ops.LAZY_GRADS[0] = False
        if share:
            old_share = ops.share_setup(False)
        yield
    finally:
        ops.LAZY_GRADS[0] = old_lazy
        if old_share is not None:
            ops.share_setup(old_share)


def grads(loss, leaves, **kw):
    """torch.autograd.grad(loss, leaves, allow_unused=True) -> (gradients with None as zeros, the raw tuple): a missing
    path then compares as a number, and `raw[i] is None` is there for where that is the claim."""
    raw = torch.autograd.grad(loss, leaves, allow_unused=True, **kw)
    return tuple(torch.zeros_like(x) if g is None else g for g, x in zip(raw, leaves)), raw


def close(got, want, rel):
    """max|got - want| <= rel * max|want|, -> (ok, the two figures)."""
    err, bar = float((got - want).abs().max()), rel * float(want.abs().max())
    return err <= bar, (err, bar)


def scene(meshes, d, name="horse", N=4, H=64, R=2, seed=41):
    """The inputs of test_gpu_dropin.py's `_inputs`: vertices / cameras (numpy, to make leaves from), faces, ground-truth
    mask, distance transform, image, boundary points, atlas."""
    rng = np.random.default_rng(seed)
    v, f = meshes[name + "_v"], meshes[name + "_f"]
    verts = batch_verts(v, N, rng, 0.01)
    cams = make_cams(N, rng, extent=float(np.abs(v).max()))
    gt = (rng.uniform(size=(N, H, H)) > 0.5).astype(np.float32)
    edt = rng.uniform(0, 3, (N, 1, H, H)).astype(np.float32)
    img = rng.uniform(0, 1, (N, 3, H, H)).astype(np.float32)
    bds = np.concatenate([rng.uniform(-0.8, 0.8, (N, 40, 2)), (rng.uniform(size=(N, 40, 1)) > 0.2)], -1).astype(np.float32)
    atlas = rng.uniform(0, 1, (N, f.shape[0], R, R, 3)).astype(np.float32)
    gt2 = (rng.uniform(size=(N, H, H)) > 0.5).astype(np.float32)
    t = lambda x: torch.tensor(x, device=d)
    return dict(N=N, H=H, verts=verts, cams=cams, gt=t(gt), gt2=t(gt2), edt=t(edt), img=t(img), bds=t(bds), atlas=atlas,
                faces=torch.from_numpy(f).to(d)[None].repeat(N, 1, 1))


def leaves(I, d, atlas=False):
    tv = torch.tensor(I["verts"], device=d, requires_grad=True)
    tc = torch.tensor(I["cams"], device=d, requires_grad=True)
    if atlas:
        return tv, tc, torch.tensor(I["atlas"], device=d, requires_grad=True)
    return tv, tc


def solver_case(meshes, d, N=5, Kh=8, seed=21):
    """test_gpu_composed.py's exchange case: bird, N = 5 frames, K_h = 8 handles.  -> (make() -> (solver, extra
    parameter), delta [N,K_h,3], two weight tensors [N,V,3] for two losses on the predicted vertices)."""
    from acfm_video_3d_reconstruction_amd.deform import DeformSolver
    rng = np.random.default_rng(seed)
    v, f = meshes["bird_v"], meshes["bird_f"]
    delta = torch.tensor(rng.normal(0, 0.02, (N, Kh, 3)).astype(np.float32), device=d)
    wa = torch.tensor(rng.normal(0, 1, (N, v.shape[0], 3)).astype(np.float32), device=d)
    wb = torch.tensor(rng.normal(0, 1, (N, v.shape[0], 3)).astype(np.float32), device=d)

    def make():
        lbs = torch.nn.Parameter(torch.tensor(fps_lbs_logits(v, Kh), device=d))
        mean = torch.nn.Parameter(torch.tensor(v, device=d))
        extra = torch.nn.Parameter(torch.tensor([0.3, -0.2], device=d))
        return DeformSolver(mean, torch.tensor(f, device=d), lbs), extra
    return make, delta, wa, wb
