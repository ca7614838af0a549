"""Restatements of TexturesUV.sample_textures shared by the UV texture tests: the composition over
grid_sample, the same written out with explicit floor and weights, and the sampling coordinates.  All of them work in
the dtype of their float inputs and are differentiable."""
import torch


def _uv(p2f, bary, fvuv):
    vals = fvuv[p2f.clamp(min=0)]                                   # [N,H,W,K,3,2]
    return (bary[..., None] * vals).sum(dim=-2) * (p2f >= 0)[..., None].to(bary.dtype)


def coords(p2f, bary, fvuv, Hm, Wm, align_corners, padding_mode):
    """-> (x, y): the sampling coordinates in texels, [N,H,W,K] each (y counted in the flipped map)."""
    uv = _uv(p2f, bary, fvuv)

    def one(t, S):
        g = 2.0 * t - 1.0
        x = (g + 1.0) / 2.0 * (S - 1) if align_corners else ((g + 1.0) * S - 1.0) / 2.0
        return x.clamp(0, S - 1) if padding_mode == "border" else x

    return one(uv[..., 0], Wm), one(uv[..., 1], Hm)


def composition(p2f, bary, fvuv, maps, align_corners=True, padding_mode="border"):
    """uv -> 2 uv - 1 -> grid_sample of the map flipped along its height; the mesh is the pixel's."""
    N, H, W, K = p2f.shape
    grid = (2.0 * _uv(p2f, bary, fvuv) - 1.0).reshape(N, H, W * K, 2)
    m = torch.flip(maps, [1]).permute(0, 3, 1, 2)
    out = torch.nn.functional.grid_sample(m, grid, mode="bilinear", padding_mode=padding_mode,
                                          align_corners=align_corners)
    return out.permute(0, 2, 3, 1).reshape(N, H, W, K, 3)


def restatement(p2f, bary, fvuv, maps, align_corners=True, padding_mode="border"):
    """The same without grid_sample: floor, the four weights, taps outside the map dropped, rows read as
    maps[n, Hm - 1 - y, x]."""
    N, Hm, Wm = maps.shape[:3]
    x, y = coords(p2f, bary, fvuv, Hm, Wm, align_corners, padding_mode)
    x0, y0 = torch.floor(x.detach()), torch.floor(y.detach())
    n = torch.arange(N).reshape(N, 1, 1, 1).expand_as(p2f)
    out = 0.0
    for dy in (0, 1):
        for dx in (0, 1):
            xi, yi = x0 + dx, y0 + dy
            wx = (x - x0) if dx else (x0 + 1.0 - x)
            wy = (y - y0) if dy else (y0 + 1.0 - y)
            ok = (xi >= 0) & (xi <= Wm - 1) & (yi >= 0) & (yi <= Hm - 1)
            row = (Hm - 1 - yi).clamp(0, Hm - 1).long()
            tex = maps[n, row, xi.clamp(0, Wm - 1).long()]
            out = out + tex * (wx * wy * ok.to(maps.dtype))[..., None]
    return out
