"""Drop-in for multiframe/data/optical_flow/model/correlation_package/correlation.py (the one
native extension of the reference tree): `Correlation(pad_size, kernel_size, max_displacement,
stride1, stride2, corr_multiply)` with the configuration MaskFlownet uses (MaskFlownet.py:116, 416:
pad_size = max_displacement, kernel_size = 1, strides 1).  Forward only (ACFM never trains the flow network) unless
`flow_ops.trainable()` is on: then GPU calls that need gradients run the backward kernel, as the reference's
CorrelationFunction.backward does (correlation.py:38-52)."""
import torch
import torch.nn.functional as F
from torch import nn

from . import ops


def correlation_torch(f1, f2, md):
    """The operator's definition in torch ops, on any device and in any float dtype: zero-pad f2 by md, take the
    (2md+1)^2 shifted products and the mean over C; channel (tj+md)(2md+1) + (ti+md) pairs f1[y,x] with f2[y+tj,x+ti].
    Differentiable like any torch expression: the tests' float64 reference and the benchmark's baseline."""
    md = int(md)
    H, W = f1.shape[-2:]
    p2 = F.pad(f2, (md, md, md, md))
    return torch.stack([(f1 * p2[..., tj:tj + H, ti:ti + W]).mean(1)
                        for tj in range(2 * md + 1) for ti in range(2 * md + 1)], 1)


class Correlation(nn.Module):
    def __init__(self, pad_size=0, kernel_size=0, max_displacement=0, stride1=1, stride2=2, corr_multiply=1):
        super().__init__()
        if kernel_size != 1 or stride1 != 1 or stride2 != 1 or pad_size != max_displacement or corr_multiply != 1 \
                or not 1 <= max_displacement <= 4:
            raise NotImplementedError(
                "Correlation: only MaskFlownet's configuration is built (kernel_size=1, stride1=stride2=1, "
                "pad_size=max_displacement in 1..4, corr_multiply=1)")
        self.pad_size, self.kernel_size, self.max_displacement = pad_size, kernel_size, max_displacement
        self.stride1, self.stride2, self.corr_multiply = stride1, stride2, corr_multiply

    def forward(self, input1, input2):
        return ops.correlation(input1, input2, self.max_displacement)
