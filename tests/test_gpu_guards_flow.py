"""GPU: the flow operators (correlation, deformable convolution) on hostile, fenced memory: tests/guards.py run_case.

What is bits and what is not follows the kernels.  correlation: the backward is two fixed-order gathers (bits); the
forward splits the channels of a small map over workgroups that add atomically (csplit > 1 in
acfm_correlation_forward), so at (1, 37, 17, 19) it is held to the float64 oracle at the existing rtol 1e-4 / atol 1e-5
in every run, and at 768 tiles (3, 16, 256, 256) -- csplit = 1, two 8-channel LDS chunks, a path no other test
reaches -- it is bits.  deform_conv2d: the forward and the offset / weight / bias gradients are bits, grad_input is
added atomically and is held to float64 autograd at the project's 1e-4 bound in every run."""
import numpy as np
import pytest
import torch

import guards
from oracle import oracle as O
from test_flow_grad import BOUND, ratio
from test_flow_ops import GPU_CASES, TOL
from test_gpu_flow_grad import _corr_case, _dconv_case

pytestmark = pytest.mark.gpu
_report = guards.module_report(__name__)

NO_SPLIT = (3, 16, 256, 256, 1)       # 16 x 16 x 3 = 768 tiles: no channel split; C = 16: two chunks of 8 channels


def _d():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, d, grad=False):
    return torch.tensor(a, device=d, requires_grad=grad)


def _no_split_inputs():
    N, C, H, W, md = NO_SPLIT
    rng = np.random.default_rng(16)
    return rng.standard_normal((N, C, H, W)).astype(np.float32), rng.standard_normal((N, C, H, W)).astype(np.float32)


def test_correlation_forward_without_channel_split():
    """The non-atomic forward (k_correlation_fwd<MD, false>) with more than one 8-channel LDS chunk, against the
    float64 oracle; two runs are the same bits."""
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    N, C, H, W, md = NO_SPLIT
    assert (W + 15) // 16 * ((H + 15) // 16) * N >= 768 and C > 8
    f1, f2 = _no_split_inputs()
    with torch.no_grad():
        out = ops.correlation(_t(f1, d), _t(f2, d), md)
        again = ops.correlation(_t(f1, d), _t(f2, d), md)
    ref = O.correlation(f1, f2, md)
    assert out.shape == ref.shape == (N, 9, H, W)
    got = out.cpu().numpy()
    print("correlation %s: max |got - oracle| = %.3g" % (NO_SPLIT, float(np.abs(got - ref).max())))
    np.testing.assert_allclose(got, ref, **TOL)
    assert torch.equal(out, again)


def test_correlation_no_split_guarded():
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    f1, f2 = _no_split_inputs()

    def fn(inp):
        with torch.no_grad():
            return dict(out=ops.correlation(inp(_t(f1, d)), inp(_t(f2, d)), NO_SPLIT[4]))
    guards.run_case(fn)


def test_correlation_small_map_forward_and_backward():
    from acfm_video_3d_reconstruction_amd import flow_ops, ops
    d = _d()
    case = (1, 37, 17, 19, 2)
    f1, f2, go, _ = _corr_case(case)
    ref = O.correlation(f1, f2, case[4])

    def fn(inp):
        t1, t2 = inp(_t(f1, d, True)), inp(_t(f2, d, True))
        with flow_ops.trainable():
            out = ops.correlation(t1, t2, case[4])
            g1, g2 = torch.autograd.grad(out, (t1, t2), inp(_t(go, d)))
        np.testing.assert_allclose(out.detach().cpu().numpy(), ref, **TOL)
        return dict(out=out, g1=g1, g2=g2)
    guards.run_case(fn, loose=("out",))


@pytest.mark.parametrize("case,shared", [(GPU_CASES[5], False), (GPU_CASES[1], False), (GPU_CASES[1], True)],
                         ids=lambda v: str(v).replace(" ", ""))
def test_deform_conv2d(case, shared):
    from acfm_video_3d_reconstruction_amd import flow_ops, ops
    d = _d()
    x, off, w, b, go, ref = _dconv_case(case, shared)

    def fn(inp):
        t = [inp(_t(a, d, True)) for a in (x, off, w, b)]
        with flow_ops.trainable():
            out = ops.deform_conv2d(*t, shared_offset=shared)
            gx, goff, gw, gb = torch.autograd.grad(out, t, inp(_t(go, d)))
        r = ratio(gx.cpu().numpy(), ref[0])
        assert r <= BOUND, ("grad_input", r)
        return dict(out=out, gx=gx, goff=goff, gw=gw, gb=gb)
    guards.run_case(fn, loose=("gx",))
