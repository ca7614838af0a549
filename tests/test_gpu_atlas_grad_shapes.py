"""GPU: the gather form of the atlas gradient (k_tex_bwd_faces) on hand-built scenes, through the public operators and
on both entry paths: an explicit image gradient (acfm_tex_backward_faces) and masked_texture_mse on the rendered image,
whose lazy gradient reaches acfm_tex_mse_backward_faces.  Scenes and cases: tools/record_atlas_grad_parent.py (boxes
under 64 pixels, between 64 pixels and one round of the walk (128) and of more than three rounds; a wave with four big
faces and one mixing big, small and invisible ones; F = 26 and F = 3; occluded, degenerate, partly and wholly outside faces; R in {1, 6, 8};
N = NA and N = 2 NA; NA = 8 (per-XCD placement) and NA = 3; a workspace taken over from a blurred silhouette render).

Reference: oracle.tex_render_backward_atlas on the render's own texel indices, summed in float64.  A texel's gradient
is a float32 sum of n addends in some order, so it lies within n 2^-23 sum|addend| of it (each of the n - 1 roundings
is at most 2^-24 of a partial sum <= sum|addend|, and the reference's own rounding to float32 is one more): derived,
not tuned, and zero for a texel no pixel shows -- exact zeros.  For the MSE path the addends are the per-pixel
gradients formed on the CPU in float32 with the kernel's expression and operation order.

Bits: the build before "two load round trips per wave, one item list per wave" gave tests/golden/atlas_grad_parent.npz
(recorded with that build's library); the addends of a texel still arrive in pixel order, so equal bits are the claim.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_atlas_grad_parent as R  # noqa: E402
from oracle import oracle as O  # noqa: E402

_RUNS = {}


def _run(i):
    """Case i on the GPU, twice (the second run for the run-to-run comparison); computed once per session."""
    if i not in _RUNS:
        calls = []
        _RUNS[i] = (R.run_case(i, R.CASES[i], calls), R.run_case(i, R.CASES[i]), calls)
    return _RUNS[i]


def _check_against_reference(ga, tidx, addends, NA):
    """ga [NA,F,R,R,3] against the float64 sum of addends [N,3,H,H] over the pixels of each texel."""
    ref = O.tex_render_backward_atlas(tidx, addends, ga.shape).astype(np.float64)
    t = tidx.reshape(-1)
    sel = t >= 0
    n_add = np.zeros(ga[..., 0].size, np.float64)
    np.add.at(n_add, t[sel], 1.0)
    sum_abs = np.zeros((ga[..., 0].size, 3), np.float64)
    np.add.at(sum_abs, t[sel], np.abs(addends.astype(np.float64)).transpose(0, 2, 3, 1).reshape(-1, 3)[sel])
    bound = (n_add[:, None] * 2.0 ** -23 * sum_abs).reshape(ga.shape)
    err = np.abs(ga.astype(np.float64) - ref)
    print("texels %d, with addends %d, most addends %d, max err %.3g, max err / bound %.3g" % (
        n_add.size, (n_add > 0).sum(), n_add.max(), err.max(), (err[bound > 0] / bound[bound > 0]).max()))
    assert (err <= bound).all()
    assert (ga.reshape(-1, 3)[n_add == 0] == 0).all()           # exact zeros where no pixel shows the texel
    return n_add.reshape(ga.shape[:-1])


@pytest.mark.parametrize("i", range(len(R.CASES)))
def test_explicit_gradient_against_the_float64_sum(i):
    kind, N, NA, H, Rr, shared = R.CASES[i]
    r, _, calls = _run(i)
    assert "acfm_tex_backward_faces" in calls
    x = R.make_inputs(i, R.CASES[i])
    n_add = _check_against_reference(r["ga_given"], r["tidx"], x["g"], NA)
    if kind == "mixed":
        assert n_add[:, 0].sum() > 3 * 256 * NA                 # the face over the whole image: more than three rounds
        for f in (2, 9, 10, 15):                                # degenerate, outside, occluded, behind the stack
            assert (n_add[:, f] == 0).all() and (r["ga_given"][:, f] == 0).all()
        assert (n_add[:, [7, 14, 21]].sum((2, 3)) > 64).all()   # the other big faces of the first wave
        assert (n_add[:, 16].sum((1, 2)) > 0).all()             # partly outside
        if N == 2 * NA:
            assert n_add.max() >= 2
        box = R.tight_boxes(x["verts"], x["faces"], H)
        assert (box[:, 0] == H * H).all() and (box[:, [7, 14, 21]] > 128).all()
        assert (box[:, [4, 5, 6, 8]] < 64).all() and (box[:, [2, 9]] == 0).all()
        if H == 40:                                             # the sliver: between 64 pixels and one round (128 items)
            assert ((box[:, 3] > 64) & (box[:, 3] <= 128)).all() and (n_add[:, 3].sum((1, 2)) > 0).all()


@pytest.mark.parametrize("i", range(len(R.CASES)))
def test_mse_gradient_against_the_float64_sum(i):
    kind, N, NA, H, Rr, shared = R.CASES[i]
    r, _, calls = _run(i)
    assert "acfm_tex_mse_backward_faces" in calls and "acfm_tex_mse_backward" not in calls
    x = R.make_inputs(i, R.CASES[i])
    f32 = np.float32
    idx = np.arange(N) % NA
    mk = x["mask"][idx][:, None]
    w = (x["wts"] * f32(2.0) / (f32(3.0) * f32(H * H)))[:, None, None, None]
    g = w * (r["imgs"] * mk - x["ref"][idx] * mk) * mk          # TexGradN's expression, operation for operation
    assert g.dtype == np.float32
    _check_against_reference(r["ga_mse"], r["tidx"], g, NA)


@pytest.mark.parametrize("i", range(len(R.CASES)))
def test_bits_of_the_parent_build_and_of_a_second_run(i):
    g = np.load(os.path.join(ROOT, "tests", "golden", "atlas_grad_parent.npz"))
    a, b, _ = _run(i)
    for path in ("given", "mse"):
        ga = a["ga_" + path]
        assert ga.dtype == np.float32 and np.abs(ga).sum() > 0
        assert np.array_equal(ga.view(np.uint32), b["ga_" + path].view(np.uint32))
        assert np.array_equal(ga.view(np.uint32), g["%s_%d" % (path, i)].view(np.uint32))
