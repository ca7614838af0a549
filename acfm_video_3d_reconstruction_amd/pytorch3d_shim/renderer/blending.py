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


def softmax_rgb_blend(colors, fragments, blend_params, znear=1.0, zfar=100.0):
    return _ops.softmax_rgb_blend(colors, fragments, blend_params, znear=znear, zfar=zfar)
