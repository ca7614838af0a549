"""Perceptual texture loss (csrc/acfm_lpips.hip)."""
import ctypes

import torch

from .. import _lib
from .base import _f32c, _ref_batch


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
        _lib.call("acfm_lpips_input_forward", i.device, i, m, N, m.shape[0], H, W, x)
        ctx.save_for_backward(m)
        return x

    @staticmethod
    def backward(ctx, gx):
        m, = ctx.saved_tensors
        g = _f32c(gx)
        N, _, H, W = g.shape
        gi = torch.empty_like(g)
        _lib.call("acfm_lpips_input_backward", g.device, g, m, N, m.shape[0], H, W, gi)
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
            _lib.call("acfm_lpips_layer_forward", a.device, a, b, w, N, Nr, a.shape[1], hw, _ptr_at(d, off), P)
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
                _lib.call("acfm_lpips_layer_backward", a.device, a, b, w, _ptr_at(g, off), P, N, Nr, a.shape[1], hw,
                          ga[l])
            if need_b[l]:   # Nr == N (checked by lpips_layers): d is symmetric, the same kernel with the roles exchanged
                gb[l] = torch.empty_like(b)
                _lib.call("acfm_lpips_layer_backward", a.device, b, a, w, _ptr_at(g, off), P, N, N, a.shape[1], hw,
                          gb[l])
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
    _lib.call("acfm_lpips_mask_weights", m.device, m, Nr, H, W, hw, len(sizes), M)
    return M


class _LpipsMaskedMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, d, M):
        dd, mm = _f32c(d), _f32c(M)
        N, P = dd.shape
        loss = torch.empty((N,), dtype=torch.float32, device=dd.device)
        _lib.call("acfm_lpips_masked_mean_forward", dd.device, dd, mm, N, mm.shape[0], P, loss)
        ctx.save_for_backward(mm)
        return loss

    @staticmethod
    def backward(ctx, gl):
        mm, = ctx.saved_tensors
        g = _f32c(gl)
        N, P = g.shape[0], mm.shape[1]
        gd = torch.empty((N, P), dtype=torch.float32, device=g.device)
        _lib.call("acfm_lpips_masked_mean_backward", g.device, g, mm, N, mm.shape[0], P, gd)
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
