"""CPU: every case of tests/dispatch_cases.py sits on the launch branch it is named for, and the shapes the suite
had before do not: the chip-sized rules are asked of the library's host queries (acfm_deform_conv2d_channel_tile,
acfm_correlation_channel_split: they launch nothing and load without a GPU), the fixed ones are mirrored in the helper
and held to the sources here.  The float64 references of the new deformable-convolution cases agree between their two
forms."""
import os
import re

import numpy as np
import pytest

import dispatch_cases as dc
from conftest import ROOT
from test_flow_ops import GPU_CASES, make_inputs, ref_grid, ref_loops

CSRC = os.path.join(ROOT, "acfm_video_3d_reconstruction_amd", "csrc")


def _lib():
    from acfm_video_3d_reconstruction_amd import _lib
    _lib.build()
    return _lib.lib()


def _source(name):
    return open(os.path.join(CSRC, name)).read()


def _constant(src, name):
    return int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))


# ------------------------------------------------------------------------------ the two queries
def test_channel_tile_query_and_the_forward_cases():
    tile = _lib().acfm_deform_conv2d_channel_tile
    for (N, Cin, Cout, H, W), (want, grid_y) in dc.DCONV_FWD.items():
        got = tile(N, H, W, Cout)
        assert got == want, ((N, Cin, Cout, H, W), got, want)
        assert (Cout + got - 1) // got == grid_y
        assert (H * W) % 32 != 0 and Cin % 8 != 0 and Cin > 8          # a partial pixel tile, a partial second chunk
        assert tile(1, H, W, Cout) == 16                               # an image of the batch run alone
    (N, _, Cout, H, W), _ = next(iter(dc.DCONV_FWD.items()))
    assert Cout == 40 and dc.DCONV_FWD[(N, 11, Cout, H, W)] == (64, 1)  # subtile 2 half full, subtile 3 past Cout
    # the gap being closed: every shape the suite had lands on the narrowest tile, the warp_correlate shapes as well
    for N, Cin, Cout, H, W, _ in GPU_CASES:
        assert tile(N, H, W, Cout) == 16, (N, Cin, Cout, H, W)
    for C, H, W in ((196, 6, 12), (32, 24, 40)):
        assert tile(2, H, W, C) == 16
    # the issue's example of a workload shape
    assert tile(8, 32, 32, 64) == 64
    # never wider than Cout needs, whatever the pixel count
    assert tile(64, 64, 64, 16) == 16 and tile(64, 64, 64, 17) == 32 and tile(64, 64, 64, 33) == 64
    # what the forward refuses
    for bad in ((0, 31, 33, 40), (8, 0, 33, 40), (8, 31, 0, 40), (8, 31, 33, 0), (8, 31, 33, 16 * 65535 + 1),
                (1, 46341, 46341, 4), (-1, 31, 33, 40)):
        assert tile(*bad) == 0, bad
    assert tile(1, 31, 33, 16 * 65535) == 64


def test_channel_split_query_and_the_correlation_cases():
    split = _lib().acfm_correlation_channel_split
    for (N, C, H, W, md), want in dc.CORR.items():
        assert split(N, C, H, W) == want, ((N, C, H, W, md), split(N, C, H, W))
    for (N, C, H, W, md) in dc.CORR_NO_SPLIT:
        assert (C + 7) // 8 == 3 and C % 8 != 0 and (H % 16 or W % 16)  # three chunks, the last partial; a partial tile
        assert split(1, C, H, W) > 1                                    # an image alone takes the atomic form
        assert split(N - 1, C, H, W) == 2                               # one tile fewer and the channels are split
    assert sorted(md for *_, md in dc.CORR_NO_SPLIT) == [2, 3, 4]
    assert [md for *_, md in dc.CORR_SPLIT] == [1]
    # the shapes the suite had: the only unsplit ones are one 8-channel chunk, or md = 1 (test_gpu_guards_flow.NO_SPLIT)
    from test_gpu_flow_grad import CORR_CASES
    from test_gpu_guards_flow import NO_SPLIT
    for N, C, H, W, md in CORR_CASES + ((1, 37, 17, 19, 2),):
        s = split(N, C, H, W)
        assert s == (C + 7) // 8, (N, C, H, W, md)      # split as far as the chunks go: atomic, or one chunk
        assert not (md == 1 and s > 1)                                  # <1, true> was never run
    assert split(*NO_SPLIT[:4]) == 1 and NO_SPLIT[4] == 1
    # the split never exceeds the chunks there are
    assert split(1, 8, 16, 16) == 1 and split(1, 9, 16, 16) == 2 and split(1, 24, 16, 16) == 3
    for bad in ((0, 19, 9, 7), (4097, 19, 9, 7), (1, 0, 9, 7), (1, 19, 0, 7), (1, 19, 9, 0)):
        assert split(*bad) == 0, bad
    assert split(4096, 19, 9, 7) == 1


def test_queries_are_the_rules_the_launches_use():
    """One copy of each rule: the launch code calls the function behind the query and holds no threshold of its own."""
    d, c = _source("acfm_dconv.hip"), _source("acfm_correlation.hip")
    assert len(re.findall(r"< 256\b", d)) == 1 and d.count("dconv_channel_tile(") == 3
    assert re.search(r"launch_dconv\(.*?\{.*?const int tco = dconv_channel_tile\(N, H, W, Cout\);", d, flags=re.S)
    assert len(re.findall(r"\b768\b", re.sub(r"//[^\n]*", "", c))) == 1 and c.count("corr_channel_split(") == 3
    assert re.search(r"acfm_correlation_forward\(.*?\{.*?const int csplit = corr_channel_split\(N, C, H, W\);", c,
                     flags=re.S)


# ------------------------------------------------------------------------------ the mirrored constants
def test_wgrad_mirror_matches_the_source_and_the_cases():
    src = _source("acfm_dconv_bwd.hip")
    assert (_constant(src, "DB_TP"), _constant(src, "DB_CC"), _constant(src, "DB_CO")) == (dc.DB_TP, dc.DB_CC, dc.DB_CO)
    body = re.search(r"static int wgrad_parts\(.*?\n}\n", src, flags=re.S).group(0)
    assert "(1024 + tiles_out - 1) / tiles_out" in body and "if (parts > total) parts = total;" in body
    assert "if (parts > 1024) parts = 1024;" in body and dc.WGRAD_TARGET == dc.WGRAD_PART_CAP == 1024
    assert "const int per = (int)(((long)tiles * N + parts - 1) / parts);" in src
    lib = _lib()
    for case, want in dc.DCONV_WGRAD.items():
        N, Cin, Cout, H, W = case
        got = dc.wgrad_split(*((N, Cin, H, W, Cout)))
        assert {k: got[k] for k in want} == want, (case, got)
        # the library's workspace is one [Cout, 9 Cin] slab per part
        assert lib.acfm_deform_conv2d_backward_workspace_bytes(N, Cin, H, W, Cout) == 4 * got["parts"] * Cout * 9 * Cin
    assert dc.wgrad_split(33, 5, 31, 33, 3)["parts"] == dc.WGRAD_PART_CAP
    # the gap being closed: in every shape the suite had each workgroup holds exactly one pixel tile
    for N, Cin, Cout, H, W, _ in GPU_CASES + ((2, 196, 196, 6, 12, 2.0), (2, 32, 32, 24, 40, 2.0), (2, 4, 4, 7, 9, 0.0)):
        got = dc.wgrad_split(N, Cin, H, W, Cout)
        assert got["per"] == 1 and got["parts"] == got["total"] and got["empty"] == 0, (N, Cin, Cout, H, W)
        assert lib.acfm_deform_conv2d_backward_workspace_bytes(N, Cin, H, W, Cout) == 4 * got["parts"] * Cout * 9 * Cin


def test_lpips_mirror_matches_the_source_and_the_cases():
    src = _source("acfm_lpips.hip")
    assert int(re.search(r"#define ACFM_LPIPS_WIDE_BELOW (\d+)", src).group(1)) == dc.LP_WIDE_BELOW
    assert src.count("if (tiles < (unsigned)LP_WIDE_BELOW)") == 2            # forward and backward
    assert _constant(src, "LP_ACC") == 4
    for (N, Nr, C, h, w), waves in dc.LPIPS.items():
        assert dc.lpips_waves(N, h, w) == waves
        assert C % 2 == 1 and C > 4 * 4 and Nr < N and (h * w) % dc.LP_TILE != 0
    N, _, _, h, w = dc.LPIPS_WIDE
    assert dc.lpips_tiles(N, h, w) == dc.LP_WIDE_BELOW and (N * h * w) % dc.LP_TILE == 36
    N, _, _, h, w = dc.LPIPS_NARROW
    assert dc.lpips_tiles(N, h, w) == 2037
    # the shapes the suite had: one on the four-wave side, at exactly 2048 full tiles of 8 channels
    from test_gpu_lpips import LAYER_SHAPES, WIDE_LAYER_SHAPE
    assert all(dc.lpips_waves(N, h, w) == 16 for N, _, _, h, w in LAYER_SHAPES)
    N, Nr, C, h, w = WIDE_LAYER_SHAPE
    assert dc.lpips_waves(N, h, w) == 4 and N == Nr and C < 16 and (h * w) % dc.LP_TILE == 0


# ------------------------------------------------------------------------------ the references of the new cases
@pytest.mark.parametrize("case", list(dc.DCONV_FWD), ids=lambda c: "x".join(map(str, c)))
def test_the_two_float64_forms_agree_on_the_new_cases(case):
    x, o18, o2, w, b = make_inputs(*dc.dconv_case6(case))
    r18, r2 = dc.dconv_refs(case)
    badd = b.astype(np.float64)[None, :, None, None]
    np.testing.assert_allclose(r18 + badd, ref_grid(x, o18, w, b), rtol=0, atol=1e-12)
    np.testing.assert_allclose(r2, ref_grid(x, o2, w), rtol=0, atol=1e-12)
    assert np.array_equal(ref_loops(x[:1], o18[:1], w), r18[:1])           # image by image: the batch adds nothing
