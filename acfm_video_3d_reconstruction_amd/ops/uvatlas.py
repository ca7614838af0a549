"""Texture head: UV image to face atlas (csrc/acfm_uvatlas.hip)."""
import torch

from .. import _lib
from .base import _f32c


class UVAtlasTable:
    """What uv_atlas needs of a constant sampler (uv_atlas_table builds it): the float32 sampler [F',T,T,2] and, on the
    GPU, the per-pixel tap lists of the backward -- pix_start [Hu*Wu+1] i32, pix_taps [n_entries] i32 (sample * 4 +
    corner, ascending inside a pixel: the summation order)."""

    def __init__(self, sampler, Hu, Wu, pix_start=None, pix_taps=None):
        self.sampler, self.Hu, self.Wu = sampler, int(Hu), int(Wu)
        self.Fp, self.T = int(sampler.shape[0]), int(sampler.shape[1])
        self.pix_start, self.pix_taps = pix_start, pix_taps
        self.n_entries = 0 if pix_taps is None else int(pix_taps.shape[0])

    @property
    def device(self):
        return self.sampler.device


def _uv_table_from_taps(tap_pixel, n_pixels):
    """tap_pixel [n_samples,4] (pixel of each sample's four taps, -1 = outside) -> (pix_start [n_pixels+1] i32,
    pix_taps [count] i32): pixel p owns pix_taps[pix_start[p]:pix_start[p+1]], entries sample * 4 + corner in ascending
    order (a stable sort by pixel of the entries in their own order)."""
    flat = tap_pixel.reshape(-1).to(torch.int64)
    entry = torch.nonzero(flat >= 0).reshape(-1)
    pix = flat[entry]
    if pix.numel() and int(pix.max()) >= n_pixels:
        raise ValueError("tap_pixel holds pixel %d, the image has %d" % (int(pix.max()), n_pixels))
    order = torch.sort(pix, stable=True).indices
    pix_start = torch.zeros(n_pixels + 1, dtype=torch.int32, device=flat.device)
    pix_start[1:] = torch.cumsum(torch.bincount(pix, minlength=n_pixels), 0)
    return pix_start, entry[order].to(torch.int32)


def uv_atlas_table(uv_sampler, Hu, Wu):
    """The table of uv_atlas for a sampler [F',T,T,2] (utils/mesh.py:206-232, any float type; kept as float32 as
    mesh_net.py:559 keeps it) and a UV image size, on the sampler's device.  Build it once per model and device, outside
    any graph capture (it sorts and sizes its lists on the host's say).  On the GPU it runs acfm_uv_atlas_taps, so the
    lists hold exactly the taps the forward kernel takes."""
    Hu, Wu = int(Hu), int(Wu)
    if uv_sampler.dim() != 4 or uv_sampler.shape[1] != uv_sampler.shape[2] or uv_sampler.shape[3] != 2 \
            or uv_sampler.shape[0] < 1 or uv_sampler.shape[1] < 1:
        raise ValueError("uv_sampler: [F',T,T,2] with F', T >= 1 expected, got %s" % (tuple(uv_sampler.shape),))
    if Hu < 2:
        raise ValueError("Hu must be at least 2 (align_corners=True spreads [-1, 1] over Hu - 1 pixels), got %d" % Hu)
    if Wu < 2:
        raise ValueError("Wu must be at least 2 (align_corners=True spreads [-1, 1] over Wu - 1 pixels), got %d" % Wu)
    if uv_sampler.is_cuda and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("uv_atlas_table cannot run inside a graph capture: build the table with uv_atlas_table "
                           "(or run the UVAtlasSampler once) before capturing")
    s = uv_sampler.detach().to(torch.float32).contiguous()
    if not bool(torch.isfinite(s).all()):
        raise ValueError("uv_sampler holds coordinates that are not finite")
    if not s.is_cuda:
        return UVAtlasTable(s, Hu, Wu)
    n = s.shape[0] * s.shape[1] * s.shape[2]
    taps = torch.empty((n, 4), dtype=torch.int32, device=s.device)
    _lib.call("acfm_uv_atlas_taps", s.device, s, n, Hu, Wu, taps)
    return UVAtlasTable(s, Hu, Wu, *_uv_table_from_taps(taps, Hu * Wu))


class _UVAtlas(torch.autograd.Function):
    @staticmethod
    def forward(ctx, uvimage, table, nsym):
        x = uvimage.detach().contiguous()
        B = x.shape[0]
        atlas = torch.empty((B, table.Fp + nsym, table.T, table.T, 3), dtype=torch.float32, device=x.device)
        _lib.call("acfm_uv_atlas_forward", x.device, x, table.sampler, B, table.Hu, table.Wu, table.Fp, table.T, nsym,
                  atlas)
        ctx.save_for_backward(atlas)
        ctx.cfg = (table, nsym)
        return atlas

    @staticmethod
    def backward(ctx, go):
        atlas, = ctx.saved_tensors
        table, nsym = ctx.cfg
        g = _f32c(go)
        B = atlas.shape[0]
        gx = torch.empty((B, 3, table.Hu, table.Wu), dtype=torch.float32, device=atlas.device)
        _lib.call("acfm_uv_atlas_backward", atlas.device, g, atlas, table.sampler, table.pix_start, table.pix_taps,
                  table.n_entries, B, table.Hu, table.Wu, table.Fp, table.T, nsym, gx)
        return gx, None, None


def uv_atlas(uvimage, table, num_sym_faces=0):
    """The tail of TexturePredictorUV.forward (mesh_net.py:169-179): uvimage [B,3,Hu,Wu] float32 -> atlas
    [B,F'+S,T,T,3] = (tanh(grid_sample(uvimage, sampler, align_corners=True)) + 1) / 2 per texel, the last S =
    num_sym_faces faces of the sampler once more behind the F'.  One launch forward, one backward (a gather per UV pixel
    over the table's lists: no atomics, bit-reproducible); nothing is allocated but the outputs, so both can be
    captured.  Host tensors run the reference's lines themselves."""
    if not isinstance(table, UVAtlasTable):
        raise ValueError("table: a UVAtlasTable (ops.uv_atlas_table(uv_sampler, Hu, Wu)) expected, got %s"
                         % type(table).__name__)
    if uvimage.dim() != 4 or uvimage.shape[1] != 3 or uvimage.shape[0] < 1:
        raise ValueError("uvimage: [B,3,Hu,Wu] expected (3 channels), got %s" % (tuple(uvimage.shape),))
    if uvimage.dtype != torch.float32:
        raise ValueError("uvimage must be float32, got %s" % uvimage.dtype)
    if tuple(uvimage.shape[2:]) != (table.Hu, table.Wu):
        raise ValueError("uvimage is %d x %d, the table was built for %d x %d"
                         % (uvimage.shape[2], uvimage.shape[3], table.Hu, table.Wu))
    nsym = int(num_sym_faces)
    if not 0 <= nsym <= table.Fp:
        raise ValueError("num_sym_faces must lie in [0, F'] = [0, %d], got %d" % (table.Fp, nsym))
    if uvimage.device != table.device:
        raise ValueError("uvimage is on %s, the table on %s" % (uvimage.device, table.device))
    if not uvimage.is_cuda:
        F_, T = table.Fp, table.T
        grid = table.sampler.view(1, F_, T * T, 2)
        tex = torch.nn.functional.grid_sample(uvimage, grid.repeat(uvimage.shape[0], 1, 1, 1), align_corners=True)
        tex = tex.reshape(uvimage.size(0), -1, F_, T, T).permute(0, 2, 3, 4, 1)
        tex = (torch.tanh(tex) + 1) / 2
        return torch.cat([tex, tex[:, F_ - nsym:]], 1) if nsym else tex
    return _UVAtlas.apply(uvimage, table, nsym)
