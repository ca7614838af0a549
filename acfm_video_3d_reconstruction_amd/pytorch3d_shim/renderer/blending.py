"""pytorch3d.renderer.blending (0.3.0): BlendParams and the three blends.  sigmoid_alpha_blend and softmax_rgb_blend
run on the HIP kernels (ops.sigmoid_alpha_blend / ops.softmax_rgb_blend); hard_rgb_blend is a
select of slot 0, written in torch."""
from typing import NamedTuple, Sequence, Union

import torch

from ... import ops as _ops


class BlendParams(NamedTuple):
    sigma: float = 1e-4
    gamma: float = 1e-4
    background_color: Union[float, Sequence[float]] = (1.0, 1.0, 1.0)


def _background(colors, blend_params):
    bg = blend_params.background_color
    bg = bg.to(colors) if torch.is_tensor(bg) else colors.new_tensor(bg)
    return bg.reshape(-1).expand(3) if bg.numel() == 1 else bg.reshape(3)


def hard_rgb_blend(colors, fragments, blend_params):
    """RGB of the nearest face, the background where pix_to_face[..., 0] < 0; alpha 1 everywhere (as in 0.3.0)."""
    is_background = fragments.pix_to_face[..., 0:1] < 0
    rgb = torch.where(is_background, _background(colors, blend_params), colors[..., 0, :])
    return torch.cat([rgb, torch.ones_like(rgb[..., :1])], dim=-1)


def sigmoid_alpha_blend(colors, fragments, blend_params):
    return _ops.sigmoid_alpha_blend(colors, fragments, blend_params)


def softmax_rgb_blend_composition(colors, fragments, blend_params, znear=1.0, zfar=100.0):
    """softmax_rgb_blend as PyTorch3D 0.3.0 composes it from torch operators: the host path."""
    eps = 1e-10
    mask = (fragments.pix_to_face >= 0).to(colors.dtype)
    prob = torch.sigmoid(-fragments.dists / blend_params.sigma) * mask
    alpha = torch.prod(1.0 - prob, dim=-1)
    z_inv = (zfar - fragments.zbuf) / (zfar - znear) * mask
    z_inv_max = torch.max(z_inv, dim=-1).values[..., None].clamp(min=eps)
    num = prob * torch.exp((z_inv - z_inv_max) / blend_params.gamma)
    delta = torch.exp((eps - z_inv_max) / blend_params.gamma).clamp(min=eps)
    denom = num.sum(dim=-1)[..., None] + delta
    rgb = ((num[..., None] * colors).sum(dim=-2) + delta * _background(colors, blend_params)) / denom
    return torch.cat([rgb, (1.0 - alpha)[..., None]], dim=-1)


def softmax_rgb_blend(colors, fragments, blend_params, znear=1.0, zfar=100.0):
    """The HIP kernel on GPU tensors; on host tensors the composition of torch operators."""
    if torch.is_tensor(colors) and not colors.is_cuda and not fragments.pix_to_face.is_cuda:
        return softmax_rgb_blend_composition(colors, fragments, blend_params, znear=znear, zfar=zfar)
    return _ops.softmax_rgb_blend(colors, fragments, blend_params, znear=znear, zfar=zfar)
