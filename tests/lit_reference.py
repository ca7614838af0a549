"""float64 restatements of the lit shading shared by test_lit_shading.py and the GPU tests (a helper,
not a test file): vertex / face normals, the lighting function, and the Phong / Gouraud / flat colours over fragments.
Everything is differentiable torch in float64 on the host."""
import numpy as np
import torch


def normalize(x, eps=1e-6):
    return x / x.norm(dim=-1, keepdim=True).clamp(min=eps)


def normals(verts, faces):
    """-> (vertex normals [V,3], face normals [F,3]) by 0.3.0's rule."""
    fv = verts[faces]
    raw = torch.zeros_like(verts)
    for i, a, b in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
        raw = raw.index_add(0, faces[:, i], torch.cross(fv[:, a] - fv[:, i], fv[:, b] - fv[:, i], dim=1))
    return normalize(raw), normalize(torch.cross(fv[:, 2] - fv[:, 1], fv[:, 0] - fv[:, 1], dim=1))


def lighting(p, n, col, amb, dif, spec, vec, point, cam, shin):
    """(ambient + diffuse relu(n.l)) col + specular relu(v.r)^shin [n.l > 0]; the constants broadcast against p."""
    nn = normalize(n)
    l = normalize(vec - p if point else vec.expand_as(p))
    c = (nn * l).sum(-1)
    v = normalize(cam - p)
    r = -l + 2.0 * c[..., None] * nn
    alpha = torch.relu((v * r).sum(-1)) * (c > 0).double()
    return (amb + dif * torch.relu(c)[..., None]) * col + spec * torch.pow(alpha, shin)[..., None]


def interpolate(p2f, bary, attrs):
    vals = attrs[p2f.clamp(min=0)]
    out = (bary[..., None] * vals).sum(-2)
    return out * (p2f >= 0)[..., None].double()


def per_mesh(t, dims):
    """[3], [1,3] or [N,3] -> float64 [N or 1, 1, ..., 3] against a tensor of `dims` axes."""
    t = torch.as_tensor(t).detach().cpu().double().reshape(-1, 3)
    return t.reshape((-1,) + (1,) * (dims - 2) + (3,))


class Light:
    """ambient / diffuse / specular products, light vector, camera centre and shininess of N meshes."""

    def __init__(self, N, amb, dif, spec, vec, point, cam, shin):
        self.N, self.point = N, bool(point)
        self.raw = dict(amb=amb, dif=dif, spec=spec, vec=vec, cam=cam)
        self.shin = shin

    def at(self, dims):
        c = {k: per_mesh(v, dims) for k, v in self.raw.items()}
        s = self.shin
        if torch.is_tensor(s) or isinstance(s, (list, tuple)):
            s = torch.as_tensor(s).detach().cpu().double().reshape((-1,) + (1,) * (dims - 2))
        return c, s


def shade(mode, verts, faces, p2f, bary, texels, light):
    """phong / flat colours [N,H,W,K,3] of packed float64 verts and texels."""
    vn, fn = normals(verts, faces)
    if mode == "phong":
        p = interpolate(p2f, bary, verts[faces])
        n = interpolate(p2f, bary, vn[faces])
    else:
        keep = (p2f >= 0)[..., None].double()
        p = verts[faces].mean(1)[p2f.clamp(min=0)] * keep
        n = fn[p2f.clamp(min=0)] * keep
    c, s = light.at(5)
    return lighting(p, n, texels, c["amb"], c["dif"], c["spec"], c["vec"], light.point, c["cam"], s)


def gouraud(verts, faces, colours, p2f, bary, light):
    """Gouraud colours: verts, colours [N,V,3] float64 lit at the vertices, then interpolated."""
    N, V = verts.shape[:2]
    vn, _ = normals(verts.reshape(-1, 3), faces)
    c, s = light.at(3)
    lit = lighting(verts, vn.reshape(N, V, 3), colours, c["amb"], c["dif"], c["spec"], c["vec"], light.point, c["cam"],
                   s)
    return interpolate(p2f, bary, lit.reshape(-1, 3)[faces])


def softmax_blend(p2f, dists, zbuf, colors, sigma, gamma, bg, znear=1.0, zfar=100.0, eps=1e-10):
    mask = (p2f >= 0).double()
    prob = torch.sigmoid(-dists / sigma) * mask
    alpha = torch.prod(1.0 - prob, dim=-1)
    z_inv = (zfar - zbuf) / (zfar - znear) * mask
    z_max = torch.max(z_inv, dim=-1).values[..., None].clamp(min=eps)
    num = prob * torch.exp((z_inv - z_max) / gamma)
    delta = torch.exp((eps - z_max) / gamma).clamp(min=eps)
    rgb = ((num[..., None] * colors).sum(-2) + delta * torch.as_tensor(bg, dtype=torch.float64)) / \
        (num.sum(-1)[..., None] + delta)
    return torch.cat([rgb, (1.0 - alpha)[..., None]], -1)


def hard_blend(p2f, colors, bg):
    rgb = torch.where(p2f[..., 0:1] < 0, torch.as_tensor(bg, dtype=torch.float64), colors[..., 0, :])
    return torch.cat([rgb, torch.ones_like(rgb[..., :1])], -1)


def fragments(N, H, W, K, Fm, seed):
    """Hand-built fragments (test_gpu_guards_other._fragments' recipe): packed ids in [-1, N Fm) of the pixel's own
    mesh, barycentrics inside the face -> (pix_to_face, zbuf, bary_coords, dists, generator)."""
    g = torch.Generator().manual_seed(seed)
    p2f = torch.randint(-1, Fm, (N, H, W, K), generator=g)
    p2f = torch.where(p2f >= 0, p2f + Fm * torch.arange(N).reshape(N, 1, 1, 1), p2f)
    bary = torch.rand(N, H, W, K, 3, generator=g) + 0.05
    bary = bary / bary.sum(-1, keepdim=True)
    zbuf = torch.where(p2f >= 0, 1.0 + torch.rand(N, H, W, K, generator=g), torch.tensor(-1.0))
    dists = torch.where(p2f >= 0, 1e-4 * torch.randn(N, H, W, K, generator=g), torch.tensor(-1.0))
    return p2f, zbuf, bary, dists, g


def close(got, ref, floor=1e-9, what="", rel_l2=1e-5, scale_bar=1e-4):
    """The project's bars (test_gpu_shaders._close): max error within scale_bar of scale, relative L2 within rel_l2."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert bool(torch.isfinite(got).all()), what + ": not finite"
    scale = float(ref.abs().max())
    err = float((got - ref).abs().max())
    print("%s: scale %.3g, max err %.3g" % (what, scale, err))
    assert err <= scale_bar * scale + floor, what
    if scale > 1e3 * floor:
        rel = float((got - ref).norm() / ref.norm())
        print("%s: relative L2 %.3g" % (what, rel))
        assert rel <= rel_l2, (what, rel)


def fan(n=64):
    """A 65-vertex fan: hub 0 of valence n, rim 1..n on a slightly domed circle -> (verts [n+1,3], faces [n,3])."""
    a = np.arange(n) * 2 * np.pi / n
    rim = np.stack([np.cos(a), np.sin(a), 0.2 * np.cos(3 * a)], 1)
    v = np.concatenate([[[0.0, 0.0, 0.5]], rim]).astype(np.float32)
    f = np.stack([np.zeros(n, np.int64), 1 + np.arange(n), 1 + (np.arange(n) + 1) % n], 1)
    return torch.from_numpy(v), torch.from_numpy(f)
