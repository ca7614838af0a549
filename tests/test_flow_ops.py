"""flow_ops (the drop-in for torchvision's DeformConv2d / deform_conv2d in MaskFlownet's configuration) on host
tensors, against a float64 restatement of the definition written here in two independent forms: direct loops over
the taps and the four corners, and nine grid_sample calls.  test_gpu_dconv.py checks the HIP kernel against the same
restatement.  Tolerance: the correlation test's (rtol 1e-4, atol 1e-5)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

TOL = dict(rtol=1e-4, atol=1e-5)

# (N, Cin, Cout, H, W, sigma): the shapes of the GPU test (test_gpu_dconv.py) and the two host shapes
GPU_CASES = ((1, 196, 196, 6, 12, 4.0), (2, 32, 32, 17, 19, 3.0), (1, 64, 96, 24, 40, 30.0), (1, 96, 7, 9, 33, 1.0),
             (3, 128, 128, 8, 8, 0.0), (1, 5, 3, 1, 1, 0.5), (1, 1, 1, 3, 50, 2.0))
HOST_CASES = ((1, 5, 3, 6, 12, 2.0), (2, 32, 32, 17, 19, 3.0))


def tile9(offset2):
    """[N,2,H,W] -> [N,18,H,W] as MaskFlownet.py:558-561 builds it: unsqueeze(1), repeat_interleave(.., 9, 1), view."""
    o = torch.repeat_interleave(torch.as_tensor(offset2).unsqueeze(1), 9, 1)
    S1, S2, S3, S4, S5 = o.shape
    return o.reshape(S1, S2 * S3, S4, S5)


@functools.lru_cache(maxsize=None)
def make_inputs(N, Cin, Cout, H, W, sigma, seed=0):
    """input ~ N(0,1), bias ~ N(0,1), weight ~ N(0,1) / sqrt(9 Cin), offsets ~ sigma N(0,1) with 18 and with 2 channels;
    float32 numpy arrays (shared between tests: do not write to them)."""
    rng = np.random.default_rng(1000 * seed + 7 * Cin + H * W)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    x, b = f(N, Cin, H, W), f(Cout)
    w = (f(Cout, Cin, 3, 3) / np.sqrt(9.0 * Cin)).astype(np.float32)
    return x, (sigma * f(N, 18, H, W)).astype(np.float32), (sigma * f(N, 2, H, W)).astype(np.float32), w, b


def ref_loops(x, offset, weight, bias=None):
    """float64, straight from the definition: for every tap the sample position, the rule that a position at or beyond
    one pixel outside gives 0, and the four neighbours floor / floor + 1 with those outside the map counted as 0."""
    x, offset, weight = (np.asarray(a, np.float64) for a in (x, offset, weight))
    N, C, H, W = x.shape
    if offset.shape[1] == 2:
        offset = np.tile(offset, (1, 9, 1, 1))
    ys, xs = np.mgrid[0:H, 0:W]
    out = np.zeros((N, weight.shape[0], H, W))
    for n in range(N):
        for t in range(9):
            ky, kx = divmod(t, 3)
            h = ys + ky - 1 + offset[n, 2 * t]
            w = xs + kx - 1 + offset[n, 2 * t + 1]
            inside = (h > -1) & (h < H) & (w > -1) & (w < W)
            h0, w0 = np.floor(h), np.floor(w)
            samp = np.zeros((C, H, W))
            for dh in (0, 1):
                for dw in (0, 1):
                    hi, wi = h0 + dh, w0 + dw
                    wt = (1.0 - np.abs(h - hi)) * (1.0 - np.abs(w - wi))
                    ok = inside & (hi >= 0) & (hi <= H - 1) & (wi >= 0) & (wi <= W - 1)
                    v = x[n][:, np.clip(hi, 0, H - 1).astype(np.int64), np.clip(wi, 0, W - 1).astype(np.int64)]
                    samp += np.where(ok, wt, 0.0)[None] * v
            out[n] += np.einsum("oc,chw->ohw", weight[:, :, ky, kx], samp)
    return out if bias is None else out + np.asarray(bias, np.float64)[None, :, None, None]


def ref_grid(x, offset, weight, bias=None):
    """float64, the other form: grid_sample(bilinear, zeros, align_corners=True) at the pixel coordinates (w, h) of every
    tap, then the contraction with the weight.  (align_corners=True has no scale for a side of one pixel: H, W >= 2.)"""
    x, offset, weight = (torch.as_tensor(np.asarray(a), dtype=torch.float64) for a in (x, offset, weight))
    N, C, H, W = x.shape
    assert H >= 2 and W >= 2
    if offset.shape[1] == 2:
        offset = tile9(offset)
    ys = torch.arange(H, dtype=torch.float64).view(1, H, 1)
    xs = torch.arange(W, dtype=torch.float64).view(1, 1, W)
    out = torch.zeros(N, weight.shape[0], H, W, dtype=torch.float64)
    for t in range(9):
        ky, kx = divmod(t, 3)
        h = ys + ky - 1 + offset[:, 2 * t]
        w = xs + kx - 1 + offset[:, 2 * t + 1]
        grid = torch.stack((2 * w / (W - 1) - 1, 2 * h / (H - 1) - 1), -1)
        s = F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
        out += torch.einsum("oc,nchw->nohw", weight[:, :, ky, kx], s)
    if bias is not None:
        out += torch.as_tensor(np.asarray(bias), dtype=torch.float64).view(1, -1, 1, 1)
    return out.numpy()


def _layer(Cin, Cout, w, b=None):
    from acfm_video_3d_reconstruction_amd.flow_ops import DeformConv2d
    m = DeformConv2d(Cin, Cout, 3, padding=1, bias=b is not None)
    m.load_state_dict({"weight": torch.tensor(w)} if b is None else {"weight": torch.tensor(w), "bias": torch.tensor(b)})
    return m


def test_the_two_float64_forms_agree():
    for case in GPU_CASES + HOST_CASES:
        if case[3] < 2 or case[4] < 2:
            continue
        x, o18, o2, w, b = make_inputs(*case)
        np.testing.assert_allclose(ref_loops(x, o18, w, b), ref_grid(x, o18, w, b), rtol=0, atol=1e-12)
        np.testing.assert_allclose(ref_loops(x, o2, w), ref_grid(x, o2, w), rtol=0, atol=1e-12)
    # the tiling of the loops form is MaskFlownet's: channel 2t is channel 0, channel 2t+1 is channel 1
    o2 = make_inputs(*HOST_CASES[0])[2]
    assert np.array_equal(np.tile(o2, (1, 9, 1, 1)), tile9(o2).numpy())
    assert np.array_equal(tile9(o2).numpy()[:, 0::2], np.repeat(o2[:, :1], 9, 1))


@pytest.mark.parametrize("case", HOST_CASES)
def test_module_on_host_tensors_equals_the_restatement(case):
    N, Cin, Cout, H, W, _ = case
    x, o18, o2, w, b = make_inputs(*case)
    with torch.no_grad():
        got = _layer(Cin, Cout, w, b)(torch.tensor(x), torch.tensor(o18))
        got_nb = _layer(Cin, Cout, w)(torch.tensor(x), torch.tensor(o18))
    assert got.shape == (N, Cout, H, W) and got.dtype == torch.float32
    np.testing.assert_allclose(got.numpy(), ref_loops(x, o18, w, b), **TOL)
    np.testing.assert_allclose(got_nb.numpy(), ref_loops(x, o18, w), **TOL)


def test_zero_offsets_equal_conv2d():
    N, Cin, Cout, H, W, _ = case = HOST_CASES[1]
    x, _, _, w, b = make_inputs(*case)
    tx = torch.tensor(x)
    with torch.no_grad():
        got = _layer(Cin, Cout, w, b)(tx, torch.zeros(N, 18, H, W))
        got2 = _layer(Cin, Cout, w, b)(tx, torch.zeros(N, 2, H, W))
    ref = F.conv2d(tx.double(), torch.tensor(w).double(), torch.tensor(b).double(), padding=1).numpy()
    np.testing.assert_allclose(got.numpy(), ref, **TOL)
    np.testing.assert_allclose(got2.numpy(), ref, **TOL)


def test_two_channel_offset_is_the_shared_form():
    N, Cin, Cout, H, W, _ = case = HOST_CASES[1]
    x, _, o2, w, b = make_inputs(*case)
    m = _layer(Cin, Cout, w, b)
    with torch.no_grad():
        shared = m(torch.tensor(x), torch.tensor(o2))
        full = m(torch.tensor(x), tile9(o2))
    np.testing.assert_allclose(shared.numpy(), full.numpy(), rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(shared.numpy(), ref_loops(x, o2, w, b), **TOL)


def test_state_dict_and_initialisation():
    from acfm_video_3d_reconstruction_amd.flow_ops import DeformConv2d
    torch.manual_seed(0)
    m = DeformConv2d(196, 64, 3, padding=1)
    sd = m.state_dict()
    assert list(sd) == ["weight", "bias"]
    assert tuple(sd["weight"].shape) == (64, 196, 3, 3) and tuple(sd["bias"].shape) == (64,)
    bound = 1.0 / np.sqrt(196 * 9)          # torch's Conv2d: kaiming_uniform_(a = sqrt 5) and the bias in +-1/sqrt(fan_in)
    assert float(sd["weight"].abs().max()) <= bound and float(sd["weight"].abs().max()) > 0.9 * bound
    assert float(sd["bias"].abs().max()) <= bound
    nb = DeformConv2d(8, 4, (3, 3), stride=(1, 1), padding=(1, 1), dilation=1, groups=1, bias=False)
    assert list(nb.state_dict()) == ["weight"] and nb.bias is None
    # a checkpoint entry of the reference's network loads as it is
    m.load_state_dict({"weight": torch.ones(64, 196, 3, 3), "bias": torch.zeros(64)})
    assert float(m.weight.detach().min()) == 1.0


def test_refusals_name_what_is_built():
    from acfm_video_3d_reconstruction_amd import flow_ops
    D = flow_ops.DeformConv2d
    for kw, word in ((dict(kernel_size=5, padding=1), "kernel_size"), (dict(kernel_size=3, padding=1, stride=2), "stride"),
                     (dict(kernel_size=3), "padding"), (dict(kernel_size=3, padding=2), "padding"),
                     (dict(kernel_size=3, padding=1, dilation=2), "dilation"),
                     (dict(kernel_size=3, padding=1, groups=2), "groups"), (dict(kernel_size=(3, 1), padding=1), "kernel_size")):
        with pytest.raises(NotImplementedError, match=word + ".*only MaskFlownet's configuration is built"):
            D(4, 4, **kw)
    m = D(4, 4, 3, padding=1)
    x = torch.zeros(1, 4, 5, 6)
    with pytest.raises(NotImplementedError, match="mask.*only MaskFlownet's configuration is built"):
        m(x, torch.zeros(1, 18, 5, 6), torch.ones(1, 9, 5, 6))
    with pytest.raises(NotImplementedError, match=r"offset of shape \(1, 36, 5, 6\).*only MaskFlownet's configuration"):
        m(x, torch.zeros(1, 36, 5, 6))
    w = torch.zeros(4, 4, 3, 3)
    f = flow_ops.deform_conv2d
    with pytest.raises(NotImplementedError, match="padding"):
        f(x, torch.zeros(1, 18, 5, 6), w)                               # torchvision's default padding=0
    with pytest.raises(NotImplementedError, match="stride"):
        f(x, torch.zeros(1, 18, 5, 6), w, padding=1, stride=2)
    with pytest.raises(NotImplementedError, match="dilation"):
        f(x, torch.zeros(1, 18, 5, 6), w, padding=1, dilation=(2, 2))
    with pytest.raises(NotImplementedError, match="kernel_size"):
        f(x, torch.zeros(1, 50, 5, 6), torch.zeros(4, 4, 5, 5), padding=1)
    with pytest.raises(NotImplementedError, match="groups"):
        f(x, torch.zeros(1, 18, 5, 6), torch.zeros(4, 2, 3, 3), padding=1)
    with pytest.raises(NotImplementedError, match="mask"):
        f(x, torch.zeros(1, 18, 5, 6), w, padding=1, mask=torch.ones(1, 9, 5, 6))
    with pytest.raises(NotImplementedError, match="offset of shape"):
        f(x, torch.zeros(1, 4, 5, 6), w, padding=1)
    with pytest.raises(ValueError, match=r"\(1, 18, 5, 7\)"):
        f(x, torch.zeros(1, 18, 5, 7), w, padding=1)


def test_functional_form_equals_the_module_and_is_differentiable_on_the_host():
    from acfm_video_3d_reconstruction_amd import flow_ops
    N, Cin, Cout, H, W, _ = case = HOST_CASES[0]
    x, o18, o2, w, b = make_inputs(*case)
    m = _layer(Cin, Cout, w, b)
    tx, to = torch.tensor(x), torch.tensor(o18)
    with torch.no_grad():
        assert torch.equal(flow_ops.deform_conv2d(tx, to, m.weight, m.bias, padding=1), m(tx, to))
        assert torch.equal(flow_ops.deform_conv2d(tx, torch.tensor(o2), m.weight, None, padding=(1, 1)),
                           _layer(Cin, Cout, w)(tx, torch.tensor(o2)))
    to.requires_grad_(True)
    m(tx, to).square().sum().backward()                               # host tensors: a plain torch expression
    assert m.weight.grad is not None and float(m.weight.grad.abs().max()) > 0
    assert to.grad is not None and float(to.grad.abs().max()) > 0
