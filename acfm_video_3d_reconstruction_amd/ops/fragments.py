"""PyTorch3D's rasterizer fragments, the shaders over them and TexturesUV texels."""
import ctypes

import torch

from .. import _lib
from .base import _a16, _f32c, _i64c, expand_faces


# ------------------------------------------------------------------------------ rasterizer fragments
FRAGMENT_K = (1, 2, 4, 8, 10, 20, 32)


class _Fragments(torch.autograd.Function):
    """PyTorch3D rasterize_meshes over NDC / view-space vertices (acfm_rasterize_fragments /
    acfm_rasterize_fragments_backward) -> (pix_to_face, zbuf, bary_coords, dists); gradients to verts_ndc only."""

    @staticmethod
    def forward(ctx, verts_ndc, faces, H, K, blur, clip):
        _lib.require_gpu(verts_ndc, faces)
        v = _f32c(verts_ndc)
        N, V, _ = v.shape
        f = expand_faces(faces, N)
        F = f.shape[1]
        dev = v.device
        p2f = torch.empty((N, H, H, K), dtype=torch.int64, device=dev)
        zbuf = torch.empty((N, H, H, K), dtype=torch.float32, device=dev)
        bary = torch.empty((N, H, H, K, 3), dtype=torch.float32, device=dev)
        dists = torch.empty((N, H, H, K), dtype=torch.float32, device=dev)
        nb = _lib.lib().acfm_rasterize_fragments_workspace_bytes(N, V, F, H)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        tune = _lib.tuning()[1]
        _lib.call("acfm_rasterize_fragments", dev, v, f, N, V, F, H, K, float(blur), int(clip), p2f, zbuf, bary, dists,
                  ws, nb, _lib.tuning_ptr(tune))
        ctx.save_for_backward(v, f, p2f)
        ctx.cfg = (H, K, float(blur), int(clip))
        ctx.ws = (ws, nb, tune)   # face records of the forward: the backward sets nothing up again
        ctx.mark_non_differentiable(p2f)
        ctx.set_materialize_grads(False)   # an unused output sends no gradient: that path is skipped, nothing read
        return p2f, zbuf, bary, dists

    @staticmethod
    def backward(ctx, _gp2f, gzbuf, gbary, gdists):
        none = (None,) * 5
        if not ctx.needs_input_grad[0] or (gzbuf is None and gbary is None and gdists is None):
            return (None,) + none
        v, f, p2f = ctx.saved_tensors
        H, K, blur, clip = ctx.cfg
        ws, nb, tune = ctx.ws
        N, V, _ = v.shape
        gz, gb, gd = (_f32c(g) if g is not None else None for g in (gzbuf, gbary, gdists))
        gv = torch.empty_like(v)
        _lib.call("acfm_rasterize_fragments_backward", v.device, v, f, p2f, gz, gb, gd, N, V, f.shape[1], H, K, blur,
                  clip, gv, ws, nb, 1, _lib.tuning_ptr(tune))
        return (gv,) + none


def rasterize_fragments(verts_ndc, faces, image_size, faces_per_pixel, blur_radius=0.0, clip_barycentric_coords=False):
    """PyTorch3D 0.3.0 rasterize_meshes (naive path) of verts_ndc [N,V,3] = (NDC x, NDC y, view z), faces [F,3] or
    [N,F,3] -> (pix_to_face [N,H,H,K] i64 packed n*F+f, zbuf [N,H,H,K], bary_coords [N,H,H,K,3], dists [N,H,H,K]),
    -1 in every empty slot.  zbuf / bary_coords / dists are differentiable with respect to verts_ndc (any subset of
    them may be used).  K = faces_per_pixel in FRAGMENT_K; raster_tuning(deterministic=True) makes the backward
    bit-reproducible."""
    H, K = int(image_size), int(faces_per_pixel)
    if K not in FRAGMENT_K:
        raise ValueError("faces_per_pixel=%d is not supported (one of %s)" % (K, FRAGMENT_K))
    if not blur_radius >= 0.0:
        raise ValueError("blur_radius must be >= 0, got %r" % (blur_radius,))
    if verts_ndc.dim() != 3 or verts_ndc.shape[-1] != 3:
        raise ValueError("verts_ndc must be [N,V,3], got %s" % (tuple(verts_ndc.shape),))
    _lib.require_gpu(verts_ndc, faces)
    return _Fragments.apply(verts_ndc, faces, H, K, float(blur_radius), bool(clip_barycentric_coords))


# ------------------------------------------------------------------------------ shaders over fragments
# PyTorch3D 0.3.0's blends and interpolate_face_attributes over Fragments: flattened to
# P = N*H*W pixels of K slots, each a call of acfm_shade.hip.  Gradients to zbuf / bary_coords / dists go back into the
# fragments, and _Fragments.backward carries them to the vertices.
def _shade_storage(storage):
    if storage != "f32":
        raise ValueError("storage=%r: half storage is not supported on the shader path (float32 only)" % (storage,))


def _frag_planes(fragments):
    """Fragments (or a (pix_to_face, zbuf, bary_coords, dists) tuple) -> the four planes.  The kernels index every
    plane by pix_to_face's [N,H,W,K] layout, so the shapes are checked here: dists / zbuf [N,H,W,K], bary_coords
    [N,H,W,K,3], K in FRAGMENT_K.  (The device is checked by the caller, after its own shape checks.)"""
    p2f, zbuf, bary, dists = (fragments.pix_to_face, fragments.zbuf, fragments.bary_coords, fragments.dists) \
        if hasattr(fragments, "pix_to_face") else tuple(fragments)
    if p2f.dim() != 4:
        raise ValueError("pix_to_face must be [N,H,W,K], got %s" % (tuple(p2f.shape),))
    K = int(p2f.shape[-1])
    if K not in FRAGMENT_K:
        raise ValueError("faces_per_pixel=%d is not supported (one of %s)" % (K, FRAGMENT_K))
    shape = tuple(p2f.shape)
    for name, t, want in (("zbuf", zbuf, shape), ("dists", dists, shape), ("bary_coords", bary, shape + (3,))):
        if t is None or tuple(t.shape) != want:
            raise ValueError("fragments.%s must be %s like pix_to_face, got %s"
                             % (name, want, None if t is None else tuple(t.shape)))
    return p2f, zbuf, bary, dists


def blend_struct(blend_params, znear=1.0, zfar=100.0):
    """BlendParams (sigma, gamma, background_color: a scalar or an RGB triple) -> the AcfmBlendParams structure."""
    bg = blend_params.background_color
    if torch.is_tensor(bg):
        bg = bg.detach().cpu().reshape(-1).tolist()
    bg = [float(bg)] * 3 if not isinstance(bg, (tuple, list)) else [float(c) for c in bg]
    if len(bg) == 1:
        bg = bg * 3
    if len(bg) != 3:
        raise ValueError("background_color must be a scalar or an RGB triple, got %r" % (blend_params.background_color,))
    if not (blend_params.sigma > 0 and blend_params.gamma > 0):
        raise ValueError("sigma and gamma must be > 0")
    return _lib.BlendParams(float(blend_params.sigma), float(blend_params.gamma), (ctypes.c_float * 3)(*bg),
                            float(znear), float(zfar))


def _det_ws(tune, n, dev):
    """Workspace of a scattering backward: 16 bytes per gradient element in deterministic mode, else none."""
    if tune is not None and tune.flags & 1:
        nb = 16 * n
        return torch.empty(nb, dtype=torch.uint8, device=dev), nb
    return None, 0


class _SigmoidBlend(torch.autograd.Function):
    """sigmoid_alpha_blend (acfm_sigmoid_alpha_blend{,_backward}) -> RGBA [N,H,W,4]; gradients to colors and dists."""

    @staticmethod
    def forward(ctx, colors, dists, p2f, sigma):
        p2f, d = _i64c(p2f), _f32c(dists)
        K = p2f.shape[-1]
        P = p2f.numel() // K
        c = _f32c(colors) if colors is not None else None
        rgba = torch.empty(p2f.shape[:-1] + (4,), dtype=torch.float32, device=p2f.device)
        tune = _lib.tuning()[1]
        _lib.call("acfm_sigmoid_alpha_blend", p2f.device, p2f, d, c, P, K, float(sigma), rgba, _lib.tuning_ptr(tune))
        ctx.save_for_backward(p2f, d)
        ctx.cfg = (P, K, float(sigma), tune)
        ctx.set_materialize_grads(False)
        return rgba

    @staticmethod
    def backward(ctx, g):
        need_c, need_d = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if g is None or not (need_c or need_d):
            return None, None, None, None
        p2f, d = ctx.saved_tensors
        P, K, sigma, tune = ctx.cfg
        gd = torch.empty_like(d) if need_d else None
        gc = torch.empty(p2f.shape + (3,), dtype=torch.float32, device=p2f.device) if need_c else None
        _lib.call("acfm_sigmoid_alpha_blend_backward", p2f.device, p2f, d, _a16(g), P, K, sigma, gd, gc,
                  _lib.tuning_ptr(tune))
        return gc, gd, None, None


class _SoftmaxBlend(torch.autograd.Function):
    """softmax_rgb_blend (acfm_softmax_rgb_blend{,_backward}) -> RGBA [N,H,W,4].  Colours: `colors` [N,H,W,K,3], or
    `atlas` [N*F,R,R,3] sampled at bary_coords (times ambient [N,3]); gradients to colors / atlas, dists and zbuf."""

    @staticmethod
    def forward(ctx, colors, atlas, dists, zbuf, bary, p2f, ambient, params):
        p2f, d, z = _i64c(p2f), _f32c(dists), _f32c(zbuf)
        K = p2f.shape[-1]
        P = p2f.numel() // K
        N, H, W = p2f.shape[:3]
        c = _f32c(colors) if colors is not None else None
        a = _f32c(atlas) if atlas is not None else None
        b = _f32c(bary) if atlas is not None else None
        am = _f32c(ambient) if ambient is not None else None
        R, Fp = (a.shape[1], a.shape[0]) if a is not None else (0, 0)
        rgba = torch.empty((N, H, W, 4), dtype=torch.float32, device=p2f.device)
        tune = _lib.tuning()[1]
        _lib.call("acfm_softmax_rgb_blend", p2f.device, p2f, d, z, b, c, a, R, Fp, am, P, K, H * W,
                  ctypes.byref(params), rgba, _lib.tuning_ptr(tune))
        ctx.save_for_backward(p2f, d, z, b, c, a, am)
        ctx.cfg = (P, K, H * W, R, Fp, params, tune)
        ctx.set_materialize_grads(False)
        return rgba

    @staticmethod
    def backward(ctx, g):
        nig = ctx.needs_input_grad
        if g is None or not (nig[0] or nig[1] or nig[2] or nig[3]):
            return (None,) * 8
        p2f, d, z, b, c, a, am = ctx.saved_tensors
        P, K, HW, R, Fp, params, tune = ctx.cfg
        gc = torch.empty_like(c) if nig[0] else None
        ga = torch.empty_like(a) if nig[1] else None
        gd = torch.empty_like(d) if nig[2] else None
        gz = torch.empty_like(z) if nig[3] else None
        ws, nb = _det_ws(tune, a.numel(), a.device) if ga is not None else (None, 0)
        _lib.call("acfm_softmax_rgb_blend_backward", p2f.device, p2f, d, z, b, c, a, R, Fp, am, P, K, HW,
                  ctypes.byref(params), _a16(g), gd, gz, gc, ga, ws, nb, _lib.tuning_ptr(tune))
        return gc, ga, gd, gz, None, None, None, None


class _Interpolate(torch.autograd.Function):
    """interpolate_face_attributes (acfm_interpolate_face_attributes{,_backward}); gradients to bary and attributes."""

    @staticmethod
    def forward(ctx, bary, attrs, p2f):
        p2f, b, fa = _i64c(p2f), _f32c(bary), _f32c(attrs)
        K = p2f.shape[-1]
        P = p2f.numel() // K
        Fp, D = fa.shape[0], fa.shape[2]
        out = torch.empty(p2f.shape + (D,), dtype=torch.float32, device=p2f.device)
        tune = _lib.tuning()[1]
        _lib.call("acfm_interpolate_face_attributes", p2f.device, p2f, b, fa, P, K, Fp, D, out, _lib.tuning_ptr(tune))
        ctx.save_for_backward(p2f, b, fa)
        ctx.cfg = (P, K, Fp, D, tune)
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    def backward(ctx, g):
        need_b, need_a = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if g is None or not (need_b or need_a):
            return None, None, None
        p2f, b, fa = ctx.saved_tensors
        P, K, Fp, D, tune = ctx.cfg
        gb = torch.empty_like(b) if need_b else None
        ga = torch.empty_like(fa) if need_a else None
        ws, nb = _det_ws(tune, fa.numel(), fa.device) if need_a else (None, 0)
        _lib.call("acfm_interpolate_face_attributes_backward", p2f.device, p2f, b, fa, _f32c(g), P, K, Fp, D, gb, ga,
                  ws, nb, _lib.tuning_ptr(tune))
        return gb, ga, None


def sigmoid_alpha_blend(colors, fragments, blend_params, storage="f32"):
    """PyTorch3D 0.3.0 sigmoid_alpha_blend -> RGBA [N,H,W,4]: RGB = colors[..., 0, :] (1 where colors is None: the
    silhouette shader builds no ones_like tensor), A = 1 - prod_k (1 - sigmoid(-dists / sigma) [pix_to_face >= 0]).
    Differentiable with respect to colors [N,H,W,K,3] and fragments.dists."""
    _shade_storage(storage)
    p2f, zbuf, bary, dists = _frag_planes(fragments)
    if colors is not None and tuple(colors.shape) != tuple(p2f.shape) + (3,):
        raise ValueError("colors must be None or [N,H,W,K,3] = %s, got %s"
                         % (tuple(p2f.shape) + (3,), tuple(colors.shape)))
    _lib.require_gpu(p2f, zbuf, bary, dists, colors)
    if not blend_params.sigma > 0:
        raise ValueError("sigma must be > 0")
    return _SigmoidBlend.apply(colors, dists, p2f, float(blend_params.sigma))


def softmax_rgb_blend(colors, fragments, blend_params, znear=1.0, zfar=100.0, storage="f32"):
    """PyTorch3D 0.3.0 softmax_rgb_blend of colors [N,H,W,K,3] -> RGBA [N,H,W,4].
    Differentiable with respect to colors, fragments.dists and fragments.zbuf (the z_max path included)."""
    _shade_storage(storage)
    p2f, zbuf, bary, dists = _frag_planes(fragments)
    if tuple(colors.shape) != tuple(p2f.shape) + (3,):
        raise ValueError("colors must be [N,H,W,K,3] = %s, got %s" % (tuple(p2f.shape) + (3,), tuple(colors.shape)))
    _lib.require_gpu(p2f, zbuf, bary, dists, colors)
    return _SoftmaxBlend.apply(colors, None, dists, zbuf, None, p2f, None, blend_struct(blend_params, znear, zfar))


def atlas_softmax_blend(atlas, fragments, blend_params, ambient=None, znear=1.0, zfar=100.0, storage="f32"):
    """TexturesAtlas.sample_textures + an ambient-only Phong + softmax_rgb_blend in one pass (the reference's texture
    configuration): atlas [N,F,R,R,3] (or packed [N*F,R,R,3]) is sampled at fragments.bary_coords inside the kernel,
    times ambient [N,3] / [1,3] / [3] (a constant: no gradient) when given.  -> RGBA [N,H,W,4]; differentiable with
    respect to atlas, fragments.dists and fragments.zbuf (not bary_coords: the texel index is an integer)."""
    _shade_storage(storage)
    p2f, zbuf, bary, dists = _frag_planes(fragments)
    _lib.require_gpu(p2f, zbuf, bary, dists, atlas, ambient)
    if atlas.dim() == 5:
        atlas = atlas.reshape((-1,) + tuple(atlas.shape[2:]))
    if atlas.dim() != 4 or atlas.shape[1] != atlas.shape[2] or atlas.shape[3] != 3:
        raise ValueError("atlas must be [N,F,R,R,3] or [N*F,R,R,3] with 3 channels, got %s" % (tuple(atlas.shape),))
    N = p2f.shape[0]
    if ambient is not None:
        if ambient.requires_grad:
            raise ValueError("ambient is a constant of the fused atlas path (no gradient); use softmax_rgb_blend")
        ambient = ambient.detach().to(torch.float32).reshape(-1, 3)
        if ambient.shape[0] not in (1, N):
            raise ValueError("ambient must be [3], [1,3] or [N,3], got %s" % (tuple(ambient.shape),))
        ambient = ambient.expand(N, 3)
    return _SoftmaxBlend.apply(None, atlas, dists, zbuf, bary, p2f, ambient, blend_struct(blend_params, znear, zfar))


def interpolate_face_attributes(pix_to_face, barycentric_coords, face_attributes):
    """PyTorch3D 0.3.0 interpolate_face_attributes: face_attributes [F_packed,3,D] -> [N,H,W,K,D] = sum_i bary_i
    face_attributes[pix_to_face, i], 0 in empty slots.  Differentiable with respect to both float inputs."""
    K = int(pix_to_face.shape[-1])
    if K not in FRAGMENT_K:
        raise ValueError("faces_per_pixel=%d is not supported (one of %s)" % (K, FRAGMENT_K))
    if face_attributes.dim() != 3 or face_attributes.shape[1] != 3 or face_attributes.shape[2] < 1:
        raise ValueError("face_attributes must be [F,3,D], got %s" % (tuple(face_attributes.shape),))
    if tuple(barycentric_coords.shape) != tuple(pix_to_face.shape) + (3,):
        raise ValueError("barycentric_coords must be %s, got %s" % (tuple(pix_to_face.shape) + (3,),
                                                                    tuple(barycentric_coords.shape)))
    _lib.require_gpu(pix_to_face, barycentric_coords, face_attributes)
    return _Interpolate.apply(barycentric_coords, face_attributes, pix_to_face)


UV_PADDING_MODES = ("border", "zeros")


class _UvTexels(torch.autograd.Function):
    """TexturesUV.sample_textures (acfm_uv_texels{,_backward}); gradients to bary, faces_verts_uvs and
    maps, each formed only when asked for."""

    @staticmethod
    def forward(ctx, bary, fvuv, maps, p2f, align, pad):
        p2f, b, fv, m = _i64c(p2f), _f32c(bary), _f32c(fvuv), _f32c(maps)
        N, H, W, K = p2f.shape
        P = N * H * W
        Fp, Hm, Wm = fv.shape[0], m.shape[1], m.shape[2]
        out = torch.empty(p2f.shape + (3,), dtype=torch.float32, device=p2f.device)
        tune = _lib.tuning()[1]
        _lib.call("acfm_uv_texels", p2f.device, p2f, b, fv, m, P, K, H * W, Fp, N, Hm, Wm, align, pad, out,
                  _lib.tuning_ptr(tune))
        ctx.save_for_backward(p2f, b, fv, m)
        ctx.cfg = (P, K, H * W, Fp, N, Hm, Wm, align, pad, tune)
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    def backward(ctx, g):
        need_b, need_fv, need_m = ctx.needs_input_grad[:3]
        if g is None or not (need_b or need_fv or need_m):
            return (None,) * 6
        p2f, b, fv, m = ctx.saved_tensors
        P, K, HW, Fp, N, Hm, Wm, align, pad, tune = ctx.cfg
        gb = torch.empty_like(b) if need_b else None
        gfv = torch.empty_like(fv) if need_fv else None
        gm = torch.empty_like(m) if need_m else None
        n_acc = (fv.numel() if need_fv else 0) + (m.numel() if need_m else 0)
        ws, nb = _det_ws(tune, n_acc, p2f.device) if n_acc else (None, 0)
        _lib.call("acfm_uv_texels_backward", p2f.device, p2f, b, fv, m, _f32c(g), P, K, HW, Fp, N, Hm, Wm, align, pad,
                  gm, gb, gfv, ws, nb, _lib.tuning_ptr(tune))
        return gb, gfv, gm, None, None, None


def uv_texels(pix_to_face, bary_coords, faces_verts_uvs, maps, align_corners=True, padding_mode="border"):
    """PyTorch3D 0.3.0 TexturesUV.sample_textures: pix_to_face [N,H,W,K], bary_coords [N,H,W,K,3],
    faces_verts_uvs [F_packed,3,2] (= verts_uvs[faces_uvs], mesh after mesh), maps [N,Hm,Wm,3] -> texels [N,H,W,K,3]
    = grid_sample(maps[n] flipped along its height, 2 uv - 1, bilinear, padding_mode, align_corners) at uv = sum_i
    bary_i faces_verts_uvs[f, i].  The map is read in place (no K-fold copy); empty slots are not zeroed, they hold
    the sample at uv = (0, 0).  Differentiable with respect to the three float inputs."""
    if pix_to_face.dim() != 4:
        raise ValueError("pix_to_face must be [N,H,W,K], got %s" % (tuple(pix_to_face.shape),))
    K = int(pix_to_face.shape[-1])
    if K not in FRAGMENT_K:
        raise ValueError("faces_per_pixel=%d is not supported (one of %s)" % (K, FRAGMENT_K))
    if tuple(bary_coords.shape) != tuple(pix_to_face.shape) + (3,):
        raise ValueError("bary_coords must be %s, got %s" % (tuple(pix_to_face.shape) + (3,),
                                                             tuple(bary_coords.shape)))
    if faces_verts_uvs.dim() != 3 or tuple(faces_verts_uvs.shape[1:]) != (3, 2) or faces_verts_uvs.shape[0] < 1:
        raise ValueError("faces_verts_uvs must be [F_packed,3,2], got %s" % (tuple(faces_verts_uvs.shape),))
    if maps.dim() != 4 or maps.shape[3] != 3 or maps.shape[0] != pix_to_face.shape[0]:
        raise ValueError("maps must be [N,Hm,Wm,3] with N = %d, got %s" % (pix_to_face.shape[0], tuple(maps.shape)))
    if padding_mode not in UV_PADDING_MODES:
        raise ValueError("padding_mode=%r is not supported (one of %s)" % (padding_mode, UV_PADDING_MODES))
    lo = 2 if align_corners else 1
    if min(maps.shape[1], maps.shape[2]) < lo or max(maps.shape[1], maps.shape[2]) > 16384:
        raise ValueError("maps must have sides in [%d, 16384]%s, got %s"
                         % (lo, " with align_corners=True" if align_corners else "", tuple(maps.shape)))
    if pix_to_face.numel() == 0:
        raise ValueError("pix_to_face is empty: %s" % (tuple(pix_to_face.shape),))
    for name, t in (("bary_coords", bary_coords), ("faces_verts_uvs", faces_verts_uvs), ("maps", maps)):
        if t.dtype != torch.float32:
            raise ValueError("%s must be float32 (half storage is not supported on the shader path), got %s"
                             % (name, t.dtype))
    _lib.require_gpu(pix_to_face, bary_coords, faces_verts_uvs, maps)
    return _UvTexels.apply(bary_coords, faces_verts_uvs, maps, pix_to_face, int(bool(align_corners)),
                           UV_PADDING_MODES.index(padding_mode))
