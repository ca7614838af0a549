"""Host side of the solve with more than 32 handles: the workspace query of the C ABI (no GPU needed to ask it) and the
reference's expression in fp32 at the handle counts of its published models, against the fp64 oracle."""
import numpy as np
import pytest
import torch

from oracle import oracle as O


def test_solve_workspace_sizes_up_to_128_handles():
    from acfm_video_3d_reconstruction_amd import _lib
    h = _lib.lib()
    b1, b32 = h.acfm_deform_solve_workspace_bytes(642, 1), h.acfm_deform_solve_workspace_bytes(642, 32)
    b33, b64 = h.acfm_deform_solve_workspace_bytes(642, 33), h.acfm_deform_solve_workspace_bytes(642, 64)
    b128 = h.acfm_deform_solve_workspace_bytes(642, 128)
    assert b64 > 0 and b128 > 0
    assert 0 < b1 == b32 < b33 == b64 < b128            # a panel of 32 handles at a time
    assert h.acfm_deform_solve_workspace_bytes(642, 129) == 0
    assert h.acfm_deform_solve_workspace_bytes(642, 0) == 0
    # the status word lies inside the smallest workspace of this V, wherever the panels end
    off = h.acfm_deform_solve_info_offset(642)
    assert off + 8 <= b1 and off % 8 == 0


@pytest.mark.parametrize("name,Kh", [("bird", 64), ("cow", 128)])
def test_reference_formula_fp32_at_64_and_128_handles(meshes, name, Kh):
    from acfm_video_3d_reconstruction_amd.deform import deform_reference_formula
    from acfm_video_3d_reconstruction_amd.synthetic import fps_lbs_logits
    v, f = torch.from_numpy(meshes[name + "_v"]), torch.from_numpy(meshes[name + "_f"])
    logits = torch.tensor(fps_lbs_logits(v.numpy(), Kh))
    delta = 0.05 * torch.randn(2, Kh, 3, generator=torch.Generator().manual_seed(Kh))
    L64 = O.laplacian_cot(v.double(), f)
    truth = O.deform_solve(logits, v, delta, L64)
    out = deform_reference_formula(logits, v, delta, L64.float())
    assert out.dtype == torch.float32
    err = float((out.double() - truth).abs().max())
    print("%s/%d: fp32 formula vs fp64, max abs %.2e" % (name, Kh, err))
    assert err < 2e-4
