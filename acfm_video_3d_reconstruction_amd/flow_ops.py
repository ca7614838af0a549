"""Drop-in for the one thing MaskFlownet takes from torchvision (`from torchvision import ops`, MaskFlownet.py:6):
`ops.DeformConv2d` and `ops.deform_conv2d`, in the configuration the network uses (MaskFlownet.py:36-37, 488-492:
kernel 3x3, stride 1, padding 1, dilation 1, groups 1, one offset group, no modulation mask).  GPU tensors take the
HIP kernel (ops.deform_conv2d; forward only, as ACFM never trains the flow network, unless `trainable()` below is on:
then calls that need gradients run the backward kernels); host tensors take the same
definition written with torch ops (nine grid_sample calls and an einsum), differentiable like any torch expression,
so the module can be built and checked without a GPU.  An offset with 2 channels is the shared form: every tap reads
the same (row, column) offset, which is what MaskFlownet's `repeat_interleave(flow.unsqueeze(1), 9, 1).view(..)`
(= `flow.repeat(1, 9, 1, 1)`) expresses.

Fine-tuning the flow network: `flow_ops.set_trainable(True)` (or `with flow_ops.trainable():`) switches the GPU path
of DeformConv2d, deform_conv2d, warp_correlate and correlation.Correlation from refusing autograd to the backward
kernels.  The switch is process-wide, read at every call, and not thread-local (nn.DataParallel's replica threads see
it); the default is off, so a frozen network never pays for saved tensors."""
import contextlib
import math

import torch
import torch.nn.functional as F
from torch import nn

from . import ops

_BUILT = ("only MaskFlownet's configuration is built (kernel_size=3, stride=1, padding=1, dilation=1, groups=1, "
          "one offset group: an offset of 18 channels, or of 2 shared by the nine taps; no mask)")


def set_trainable(flag):
    """Turn the backward kernels of the flow operators on or off for the whole process -> the previous value."""
    previous, ops._FLOW_TRAINABLE[0] = ops._FLOW_TRAINABLE[0], bool(flag)
    return previous


def is_trainable():
    return ops._FLOW_TRAINABLE[0]


@contextlib.contextmanager
def trainable(flag=True):
    """with flow_ops.trainable(): ...   -- set_trainable(flag) for the block, the previous value afterwards."""
    previous = set_trainable(flag)
    try:
        yield
    finally:
        set_trainable(previous)


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def _refuse_config(who, kernel_size, stride, padding, dilation, groups):
    for name, got, want in (("kernel_size", kernel_size, 3), ("stride", stride, 1), ("padding", padding, 1),
                            ("dilation", dilation, 1)):
        if _pair(got) != (want, want):
            raise NotImplementedError("%s: %s=%r: %s" % (who, name, got, _BUILT))
    if groups != 1:
        raise NotImplementedError("%s: groups=%r: %s" % (who, groups, _BUILT))


def _refuse_call(who, offset, mask):
    if mask is not None:
        raise NotImplementedError("%s: a modulation mask was given: %s" % (who, _BUILT))
    if offset.dim() != 4 or offset.shape[1] not in (18, 2):
        raise NotImplementedError("%s: offset of shape %s: %s" % (who, tuple(offset.shape), _BUILT))


def deform_conv2d_torch(input, offset, weight, bias=None):
    """The operator's definition in torch ops, on any device: tap t = 3 ky + kx samples input at
    (y + ky - 1 + offset[:, 2t], x + kx - 1 + offset[:, 2t+1]) bilinearly with zeros outside (grid_sample with
    align_corners=True on the map padded by one ring of zeros, so that a map of one pixel has a scale too), and the
    nine sampled stacks are contracted with weight [Cout,Cin,3,3]."""
    N, C, H, W = input.shape
    shared = offset.shape[1] == 2
    offset = offset.to(input.dtype)
    xp = F.pad(input, (1, 1, 1, 1))
    ys = torch.arange(H, dtype=input.dtype, device=input.device).view(1, H, 1)
    xs = torch.arange(W, dtype=input.dtype, device=input.device).view(1, 1, W)
    cols = []
    for t in range(9):
        ky, kx = divmod(t, 3)
        h = ys + (ky - 1) + offset[:, 0 if shared else 2 * t]
        w = xs + (kx - 1) + offset[:, 1 if shared else 2 * t + 1]
        grid = torch.stack((2.0 * (w + 1.0) / (W + 1) - 1.0, 2.0 * (h + 1.0) / (H + 1) - 1.0), -1)
        cols.append(F.grid_sample(xp, grid, mode="bilinear", padding_mode="zeros", align_corners=True))
    out = torch.einsum("ock,nckhw->nohw", weight.reshape(weight.shape[0], C, 9).to(input.dtype), torch.stack(cols, 2))
    return out if bias is None else out + bias.to(input.dtype).view(1, -1, 1, 1)


def _run(input, offset, weight, bias):
    if input.is_cuda:
        return ops.deform_conv2d(input, offset, weight, bias, shared_offset=offset.shape[1] == 2)
    if input.dim() != 4 or weight.dim() != 4 or weight.shape[1] != input.shape[1] or \
            tuple(offset.shape) != (input.shape[0], offset.shape[1]) + tuple(input.shape[2:]):
        raise ValueError("deform_conv2d: input %s, offset %s and weight %s do not fit together"
                         % (tuple(input.shape), tuple(offset.shape), tuple(weight.shape)))
    return deform_conv2d_torch(input, offset, weight, bias)


def deform_conv2d(input, offset, weight, bias=None, stride=1, padding=0, dilation=1, mask=None):
    """torchvision.ops.deform_conv2d (note its default padding=0, which is refused: MaskFlownet passes 1)."""
    if weight.dim() != 4:
        raise ValueError("deform_conv2d: weight must be [Cout,Cin,3,3], got %s" % (tuple(weight.shape),))
    groups = input.shape[1] // max(int(weight.shape[1]), 1) if input.dim() == 4 else 1
    _refuse_config("deform_conv2d", tuple(weight.shape[2:]), stride, padding, dilation, groups)
    _refuse_call("deform_conv2d", offset, mask)
    return _run(input, offset, weight, bias)


class DeformConv2d(nn.Module):
    """torchvision.ops.DeformConv2d: the same constructor, parameters `weight` [Cout,Cin,3,3] and `bias` [Cout] under
    the same state-dict keys and initialised as torch's Conv2d does, so a MaskFlownet checkpoint loads unchanged."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True):
        super().__init__()
        _refuse_config("DeformConv2d", kernel_size, stride, padding, dilation, groups)
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride, self.padding, self.dilation = (3, 3), (1, 1), (1, 1), (1, 1)
        self.groups = groups
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, 3, 3))
        if bias:
            self.bias = nn.Parameter(torch.empty(out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if self.bias is not None:
            bound = 1.0 / math.sqrt(self.weight.shape[1] * 9)
            nn.init.uniform_(self.bias, -bound, bound)

    def forward(self, input, offset, mask=None):
        _refuse_call("DeformConv2d", offset, mask)
        return _run(input, offset, self.weight, self.bias)

    def extra_repr(self):
        return "%d, %d, kernel_size=(3, 3), stride=(1, 1), padding=(1, 1)%s" % (
            self.in_channels, self.out_channels, "" if self.bias is not None else ", bias=False")


def warp_correlate(c1, c2, flow, deform, md):
    """One pyramid level's warp and cost volume (MaskFlownet.py:558-564 and the four blocks after it):
    warp = leaky_relu(deform(c2, flow)), with flow [B,2,H,W] (the reference's `flow * self.scale / stride`) handed over
    as the shared offset instead of its ninefold copy, then leaky_relu(correlation(c1, warp, md)); both slopes 0.1.
    Under `trainable()` gradients reach c1, c2, flow and the layer's parameters."""
    warp = F.leaky_relu(deform(c2, flow), 0.1)
    return F.leaky_relu(ops.correlation(c1, warp, md), 0.1)
