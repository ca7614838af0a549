"""Host only: the rules of ops.PendingTerm that need no GPU -- what launches a deferred loss term (any read of it)
and what does not (questions about its shape and type), the refusal to compute on an input written in place since
the call, and where terms are not deferred at all."""
import threading

import pytest
import torch

from acfm_video_3d_reconstruction_amd import ops


class _Job:
    """Stands in for ops._PendingJob: counts its launches and fills the output like a kernel would."""

    def __init__(self, out):
        self.out, self.done, self.launches = out, False, 0

    def flush(self):
        if not self.done:
            self.done = True
            self.launches += 1
            self.out.fill_(2.0)


def _term(shape=(3, 4)):
    out = torch.full(shape, float("nan"))
    job = _Job(out)
    return ops.PendingTerm(out, job), job


def test_questions_about_the_tensor_do_not_launch():
    t, job = _term()
    assert t.shape == (3, 4) and t.dim() == 2 and t.size(0) == 3 and t.numel() == 12 and t.dtype == torch.float32
    assert t.device.type == "cpu" and not t.is_cuda and not t.requires_grad and t.grad_fn is None
    assert t.data_ptr() == job.out.data_ptr() and t.is_contiguous() and t._version == job.out._version
    assert t.is_pending and job.launches == 0


@pytest.mark.parametrize("use", [
    lambda t: t + 1, lambda t: 0.1 * t, lambda t: t.sum(), lambda t: t[0, 0].item(), lambda t: t[:, 0], lambda t: t.cpu(),
    lambda t: repr(t), lambda t: t.detach(), lambda t: torch.stack([t, t]), lambda t: t.mean().backward() if t.requires_grad
    else t.mean(), lambda t: t.tolist(), lambda t: t.numpy(), lambda t: torch.equal(t, t), lambda t: t.reshape(-1)])
def test_every_read_launches_once_and_sees_the_values(use):
    t, job = _term()
    r = use(t)
    assert job.launches == 1 and not t.is_pending
    if torch.is_tensor(r):
        assert (r is t or type(r) is torch.Tensor) and not torch.isnan(r).any()   # (t.cpu() of a host tensor is t)
    use(t)
    assert job.launches == 1


def test_saved_by_another_autograd_node():
    class Produce(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            out = torch.full((3,), float("nan"))
            ctx.job = _Job(out)
            return ops.PendingTerm(out, ctx.job)

        @staticmethod
        def backward(ctx, g):
            ctx.job.flush()
            return g * 3.0

    x = torch.ones(3, requires_grad=True)
    y = Produce.apply(x)
    assert type(y) is ops.PendingTerm and y.grad_fn is not None and y.is_pending
    z = y * y                       # mul saves y: it must hold the values
    assert not y.is_pending and torch.equal(z.detach(), torch.full((3,), 4.0))
    z.sum().backward()
    assert torch.equal(x.grad, torch.full((3,), 12.0))


def test_input_written_in_place_is_refused_by_name():
    job = object.__new__(ops._PendingJob)
    m = torch.zeros(4)
    job.what, job.inputs, job.done = "mask_losses", [("mask", m, m._version), ("gt", m.clone(), 0)], False
    job.device, job.kind = m.device, "mask"
    m.add_(1.0)
    with pytest.raises(RuntimeError, match="mask_losses: `mask` was written in place"):
        job.check()
    with pytest.raises(RuntimeError, match="`mask`"):
        job.flush()
    assert not job.done              # still pending: every later use raises as well


def test_switch_and_worker_threads():
    assert ops._deferring()
    with ops.defer_losses(False):
        assert not ops._deferring()
        with ops.defer_losses(True):
            assert ops._deferring()
        assert not ops._deferring()
    assert ops._deferring()
    seen = []
    th = threading.Thread(target=lambda: seen.append(ops._deferring()))   # as nn.DataParallel runs its replicas
    th.start()
    th.join()
    assert seen == [False]


def test_flush_pending_losses_and_invalidate_setups_launch_what_is_registered():
    class Reg(_Job):
        __hash__ = object.__hash__

    a, b = Reg(torch.zeros(2)), Reg(torch.zeros(2))
    with ops._LOCK:
        ops._PENDING.add(a)
        ops._PENDING.add(b)
    ops.flush_pending_losses()
    assert a.launches == 1 and b.launches == 1
    c = Reg(torch.zeros(2))
    with ops._LOCK:
        ops._PENDING.add(c)
    ops.invalidate_setups()
    assert c.launches == 1
    with ops._LOCK:
        ops._PENDING.clear()
