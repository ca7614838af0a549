"""On-device versions of the mask preparation of multiframe/utils/image.py (same function
names; masks stay on the GPU instead of the reference's numpy / device->host round trip,
multiframe/main.py:365-377)."""
import torch

from . import _lib


def _masks3(mask):
    m = mask.detach().to(torch.float32)
    if m.dim() == 2:
        m = m[None]
    return m.contiguous()


def compute_dt(mask, norm=True):
    """image.py:94-102: distance_transform_edt(1 - mask), optionally / max(H, W).
    mask [H,W] or [N,H,W] (0/1) on the GPU -> same shape, float32."""
    _lib.require_gpu(mask)
    m = _masks3(mask)
    N, H, W = m.shape
    out = torch.empty_like(m)
    nb = _lib.lib().acfm_edt_workspace_bytes(N, H, W)
    ws = torch.empty(nb, dtype=torch.uint8, device=m.device)
    divisor = max(H, W) if norm else 1
    _lib.call("acfm_edt", m.device, m, N, H, W, int(divisor), out, ws, nb)
    return out[0] if mask.dim() == 2 else out


def compute_dt_barrier(mask, k=50):
    """image.py:105-116: sigmoid(k * (dt_out - dt_in) / max(H, W))."""
    m = _masks3(mask)
    H, W = m.shape[-2:]
    diff = (compute_dt(m, norm=False) - compute_dt(1.0 - m, norm=False)) / max(H, W)
    out = 1.0 / (1.0 + torch.exp(k * -diff))
    return out[0] if mask.dim() == 2 else out


def compute_boundaries(masks, cap=None, return_counts=False):
    """image.py:122-146: masks [N,H,W] -> float32 [N, max_count, 3] = (x, y, valid) of the
    boundary pixels (find_boundaries, mode='thick'), padded to the longest list of the batch.
    One small device->host read (the counts) sizes the result, like the reference's max().

    cap: the fixed-shape form, [N, cap, 3] -- the first `cap` points of every list in row-major order, padded with
    (-1, -1, 0); no host read (so the call can be captured into a hipGraph) and no scratch beyond the result.
    return_counts: also the TRUE counts, int32 [N] on the device (a count above cap tells of the overflow)."""
    _lib.require_gpu(masks)
    m = _masks3(masks)
    N, H, W = m.shape
    fixed = cap is not None
    cap = int(cap) if fixed else H * W
    if cap <= 0:
        raise ValueError("compute_boundaries: cap must be positive")
    out = torch.empty((N, cap, 3), dtype=torch.float32, device=m.device)
    counts = torch.empty((N,), dtype=torch.int32, device=m.device)
    _lib.call("acfm_boundaries", m.device, m, N, H, W, cap, out, counts)
    if not fixed:
        max_bd = int(counts.max().item())
        out = out[:, :max_bd].contiguous()
    return (out, counts) if return_counts else out
