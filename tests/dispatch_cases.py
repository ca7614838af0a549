"""The cases of tests/test_dispatch_cases.py (CPU) and tests/test_gpu_dispatch_reach.py (GPU): shapes at which a host
function of csrc/ picks the template instantiation, or the loop shape, that the tiny shapes of the rest of the suite
never pick.  A helper, not a conftest and not a test module.

Two of the rules are sized to the chip and may be retuned: the channel tile of the deformable convolution ("a workgroup
per compute unit") and the channel split of the correlation ("768 tiles").  Those are asked of the library itself
(acfm_deform_conv2d_channel_tile, acfm_correlation_channel_split: host only, they load without a GPU), never restated
here.  The other two are fixed constants of the sources and are mirrored below, the way knn_cases.py mirrors the
k-NN thresholds: wgrad_parts of csrc/acfm_dconv_bwd.hip and LP_WIDE_BELOW of csrc/acfm_lpips.hip.
test_dispatch_cases.py holds the mirrors to the sources and every case to the branch it is named for."""
import functools

import numpy as np

# ------------------------------------------------------------------------------ deformable convolution, forward
# (N, Cin, Cout, H, W) -> (channel tile, grid.y).  31 x 33 = 1023 pixels: 32 pixel tiles per image, the last one short
# of one pixel; Cin = 11: two 8-channel chunks, the second with 3 live channels.
DCONV_SIGMA = 3.0
DCONV_FWD = {
    (8, 11, 40, 31, 33): (64, 1),    # subtile 2 holds 8 channels, subtile 3 lies wholly past Cout
    (4, 11, 70, 31, 33): (64, 2),    # the second channel tile holds 6 channels
    (8, 11, 24, 31, 33): (32, 1),
    (4, 11, 40, 31, 33): (32, 2),
}

# ------------------------------------------------------------------------------ deformable convolution, weight gradient
DB_TP, DB_CC, DB_CO = 32, 16, 64             # pixels per tile, input channels per chunk, output channels per workgroup
WGRAD_TARGET = WGRAD_PART_CAP = 1024


def wgrad_split(N, Cin, H, W, Cout):
    """wgrad_parts and the launch around it restated -> dict(tiles, tiles_out, total, parts, per, empty, crossing):
    `tiles` pixel tiles per image, `total` of them in the batch, dealt to `parts` workgroups per (Cin, Cout) tile in
    runs of `per`; `empty` parts get no tile and store zeros; `crossing` parts hold tiles of two images."""
    tiles = (H * W + DB_TP - 1) // DB_TP
    total = tiles * N
    tiles_out = ((Cin + DB_CC - 1) // DB_CC) * ((Cout + DB_CO - 1) // DB_CO)
    parts = max(1, min((WGRAD_TARGET + tiles_out - 1) // tiles_out, total, WGRAD_PART_CAP))
    per = (total + parts - 1) // parts
    runs = [(p * per, min(total, p * per + per)) for p in range(parts)]
    return dict(tiles=tiles, tiles_out=tiles_out, total=total, parts=parts, per=per,
                empty=sum(lo >= hi for lo, hi in runs),
                crossing=sum(lo < hi and lo // tiles != (hi - 1) // tiles for lo, hi in runs))


# (N, Cin, Cout, H, W) -> what wgrad_split must say.  The first two are per = 2 with 32 tiles per image: every workgroup
# adds two tiles, none straddles two images.  31 x 31 has 31 tiles per image (the last holds one pixel): with per = 2
# every other image boundary falls inside a workgroup.
DCONV_WGRAD = {
    (5, 64, 128, 31, 33): dict(tiles_out=8, parts=128, total=160, per=2, empty=48, crossing=0),
    (33, 5, 3, 31, 33): dict(tiles_out=1, parts=1024, total=1056, per=2, empty=496, crossing=0),
    (5, 64, 128, 31, 31): dict(tiles_out=8, parts=128, total=155, per=2, empty=50, crossing=2),
}

# ------------------------------------------------------------------------------ correlation
# (N, C, H, W, md) -> channel split.  9 x 7 is one partial 16 x 16 tile per image: 768 images are 768 tiles; C = 19 is
# three 8-channel chunks, the last with 3 channels.
CORR_NO_SPLIT = {(768, 19, 9, 7, 4): 1, (768, 19, 9, 7, 3): 1, (768, 19, 9, 7, 2): 1}
CORR_SPLIT = {(1, 19, 17, 33, 1): 3}
CORR = {**CORR_NO_SPLIT, **CORR_SPLIT}

# ------------------------------------------------------------------------------ LPIPS layer
LP_WIDE_BELOW = 2048                         # fewer 64-pixel tiles than this: sixteen waves per tile, else four
LP_TILE = 64


def lpips_tiles(N, h, w):
    return (N * h * w + LP_TILE - 1) // LP_TILE


def lpips_waves(N, h, w):
    return 16 if lpips_tiles(N, h, w) < LP_WIDE_BELOW else 4


# (N, Nr, C, h, w) -> waves.  181 x 181 x 4 = 131044 pixels: 2048 tiles, the last with 36 pixels; hw = 32761 is odd, so
# every image boundary falls inside a tile; C = 19 is odd and more than one round of 4 waves x 4 sums; Nr < N.
LPIPS_WIDE = (4, 2, 19, 181, 181)
LPIPS_NARROW = (4, 2, 19, 180, 181)          # 2037 tiles: its neighbour on the sixteen-wave side
LPIPS = {LPIPS_WIDE: 4, LPIPS_NARROW: 16}


# ------------------------------------------------------------------------------ inputs and references, computed once
def dconv_case6(case, sigma=DCONV_SIGMA):
    """(N, Cin, Cout, H, W) -> the six-tuple test_flow_ops.make_inputs takes."""
    return tuple(case) + (sigma,)


@functools.lru_cache(maxsize=None)
def dconv_refs(case):
    """float64 restatement (test_flow_ops.ref_loops) of a forward case without bias, for the 18-channel and for the
    2-channel offset -> (ref18, ref2); shared between the tests, do not write to them."""
    from test_flow_ops import make_inputs, ref_loops
    x, o18, o2, w, _ = make_inputs(*dconv_case6(case))
    return ref_loops(x, o18, w), ref_loops(x, o2, w)


@functools.lru_cache(maxsize=None)
def corr_inputs(case):
    """f1, f2 ~ N(0,1) float32 [N,C,H,W] of a correlation case (shared: do not write to them)."""
    N, C, H, W, md = case
    rng = np.random.default_rng(7000 + 13 * C + H * W + md)
    return rng.standard_normal((N, C, H, W)).astype(np.float32), rng.standard_normal((N, C, H, W)).astype(np.float32)
