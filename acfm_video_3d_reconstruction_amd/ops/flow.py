"""The flow operators: optical-flow loss, correlation, deformable convolution."""
import torch

from .. import _lib
from .base import _f32c


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
        _lib.call("acfm_of_loss", p.device, p, fl, mk, vi, B, T, V, H, W, clips, int(bool(flip_t)), loss, cnt)
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
        _lib.call("acfm_of_loss_backward", p.device, p, fl, mk, vi, cnt, g, B, T, V, H, W, clips, flip_t, gp)
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
_FLOW_TRAINABLE = [False]

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
    _lib.call("acfm_correlation_forward", a.device, a, b, N, C, H, W, md, out)
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
        _lib.call("acfm_correlation_backward", a.device, go, a, b, N, C, H, W, ctx.md, g1, g2)
        return (None if g1 is None else g1.to(ctx.dtypes[0]), None if g2 is None else g2.to(ctx.dtypes[1]), None)


def correlation(f1, f2, max_displacement):
    """Cost volume of MaskFlownet's Correlation layer (pad = max_displacement = md, kernel 1, strides 1):
    f1, f2 [N,C,H,W] -> [N,(2md+1)^2,H,W].  Forward only (the flow network is frozen in ACFM) unless
    `flow_ops.trainable()` is on: then a call that needs gradients goes through the backward kernel
    (acfm_correlation_backward: both sides are fixed-order gathers, bit-reproducible), with the same forward bits."""
    if torch.is_grad_enabled() and (f1.requires_grad or f2.requires_grad):
        _lib.require_gpu(f1, f2)
        if not _FLOW_TRAINABLE[0]:
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
    _lib.call("acfm_deform_conv2d_forward", x.device, x, o, w, b, N, Cin, H, W, Cout, 1 if shared_offset else 0, out)
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
        _lib.call("acfm_deform_conv2d_backward", x.device, go, x, o, w, N, Cin, H, W, Cout, 1 if ctx.shared else 0, gx,
                  goff, gw, gb, ws, nbytes)
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
        if not _FLOW_TRAINABLE[0]:
            raise RuntimeError(_FORWARD_ONLY % "deform_conv2d")
        return _DeformConv2d.apply(input, offset, weight, bias, bool(shared_offset))
    return _dconv_forward(*_dconv_args(input, offset, weight, bias, shared_offset), shared_offset)
