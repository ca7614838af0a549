"""CPU: the texture head's public layer (acfm_video_3d_reconstruction_amd/texture.py) against the fixture that
tests/golden/make_golden_uv_atlas.py took from the reference, the host path of ops.uv_atlas, the transposition of the
tap table, and the refusals."""
import numpy as np
import pytest
import torch

from conftest import load_golden


@pytest.fixture(scope="module")
def gold():
    return load_golden("uv_atlas")


def test_compute_uvsampler_matches_the_reference(gold):
    from acfm_video_3d_reconstruction_amd import texture
    nf = int(gold["num_indept_faces"]) + int(gold["num_sym_faces"])
    assert nf == 656 and gold["faces"].shape == (1280, 3)
    for T in (2, 6):
        uv = texture.compute_uvsampler(gold["verts"], gold["faces"][:nf], tex_size=T)
        want = gold["sampler_t%d" % T]
        assert uv.dtype == np.float64 and uv.shape == want.shape == (nf, T, T, 2)
        err = np.abs(uv - want).max()
        print("tex_size %d: max |uv - reference| = %.3e" % (T, err))
        assert err <= 1e-12
    # the fixture does hold samples on the border rows (case 1 of the GPU tests leans on them)
    v = gold["sampler_t6"][..., 1]
    assert (v == 1.0).sum() >= 1 and (v == -1.0).sum() >= 1
    assert texture.uv_image_size(656, 6) == (128, 256)
    assert texture.uv_image_size(656, 2) == (32, 64)


def test_spherical_coords_axes():
    from acfm_video_3d_reconstruction_amd import texture
    X = np.array([[0, 0, 2.0], [0, 0, -3.0], [1.0, 0, 0], [0, 1.0, 0], [-1.0, 1e-300, 0]])
    uv = texture.get_spherical_coords(X)
    assert np.allclose(uv[:, 1], [-1, 1, 0, 0, 0], atol=1e-15)
    assert np.allclose(uv[2:, 0], [0, 0.5, 1], atol=1e-15)


def test_host_module_equals_the_golden_atlas_bit_for_bit(gold):
    from acfm_video_3d_reconstruction_amd.texture import UVAtlasSampler
    S = int(gold["num_sym_faces"])
    uvimage = torch.from_numpy(gold["uvimage"])
    want = torch.from_numpy(gold["atlas_t2"])
    sampler = torch.from_numpy(gold["sampler_t2"])
    m = UVAtlasSampler(sampler, symmetric=True, num_sym_faces=S)
    assert "uv_sampler" in dict(m.named_buffers()) and m.uv_sampler.dtype == torch.float32
    assert torch.equal(m(uvimage), want)
    # the reference's batched sampler [B,F',T,T,2]: row 0 is kept
    mb = UVAtlasSampler(sampler.float()[None].repeat(3, 1, 1, 1, 1), symmetric=True, num_sym_faces=S)
    assert torch.equal(mb(uvimage), want)
    # symmetric=False ignores num_sym_faces (the reference passes -1) and returns the F' faces alone
    plain = UVAtlasSampler(sampler, symmetric=False, num_sym_faces=-1)(uvimage)
    assert torch.equal(plain, want[:, :656])
    # autograd runs through the host path
    x = uvimage.clone().requires_grad_(True)
    m(x).sum().backward()
    assert x.grad is not None and torch.isfinite(x.grad).all() and float(x.grad.abs().max()) > 0


def _check_table(tap_pixel, n_pixels):
    from acfm_video_3d_reconstruction_amd import ops
    start, taps = ops._uv_table_from_taps(torch.tensor(tap_pixel, dtype=torch.int32), n_pixels)
    assert start.dtype == torch.int32 and taps.dtype == torch.int32
    start, taps = start.tolist(), taps.tolist()
    flat = np.asarray(tap_pixel).reshape(-1)
    assert len(start) == n_pixels + 1 and start[0] == 0 and start[-1] == len(taps) == int((flat >= 0).sum())
    assert sorted(taps) == [int(i) for i in np.nonzero(flat >= 0)[0]]          # each live tap once, no -1 tap at all
    for p in range(n_pixels):
        mine = taps[start[p]:start[p + 1]]
        assert all(flat[e] == p for e in mine)                                  # under its own pixel
        assert mine == sorted(mine)                                             # ascending by sample (and corner)
        assert len(mine) == int((flat == p).sum())                              # (empty ranges where nothing falls)
    return start, taps


def test_table_from_taps():
    # 5 samples on a 2 x 3 image: pixel 4 collects three samples, pixel 3 nothing, sample 2 lies outside altogether
    tp = [[0, 1, 4, 5], [4, -1, 2, -1], [-1, -1, -1, -1], [1, 4, -1, 0], [5, 5, 5, 5]]
    start, taps = _check_table(tp, 6)
    assert start == [0, 2, 4, 5, 5, 8, 13]
    assert taps[start[4]:start[5]] == [2, 4, 13]
    assert taps[start[5]:start[6]] == [3, 16, 17, 18, 19]
    # nothing inside at all; and a pile-up in sample order
    start, taps = _check_table([[-1, -1, -1, -1]] * 3, 4)
    assert start == [0] * 5 and taps == []
    rng = np.random.default_rng(5)
    _check_table(rng.integers(-1, 7, size=(40, 4)).tolist(), 7)
    with pytest.raises(ValueError, match="tap_pixel"):
        _check_table([[0, 1, 2, 9]], 6)


def test_refusals_name_the_argument(gold):
    from acfm_video_3d_reconstruction_amd import ops
    from acfm_video_3d_reconstruction_amd.texture import UVAtlasSampler, compute_uvsampler
    sampler = torch.from_numpy(gold["sampler_t2"])
    m = UVAtlasSampler(sampler)
    with pytest.raises(ValueError, match="uvimage.*3 channels"):
        m(torch.zeros(2, 4, 32, 64))
    with pytest.raises(ValueError, match="uvimage.*float32"):
        m(torch.zeros(2, 3, 32, 64, dtype=torch.float64))
    with pytest.raises(ValueError, match="Hu"):
        m(torch.zeros(2, 3, 1, 64))
    with pytest.raises(ValueError, match="Wu"):
        ops.uv_atlas_table(sampler, 8, 1)
    for bad in (0, 657, None):
        with pytest.raises(ValueError, match="num_sym_faces"):
            UVAtlasSampler(sampler, symmetric=True, num_sym_faces=bad)
    UVAtlasSampler(sampler, symmetric=True, num_sym_faces=656)
    with pytest.raises(ValueError, match="uv_sampler"):
        UVAtlasSampler(sampler[:, :, :1])
    table = ops.uv_atlas_table(sampler, 32, 64)
    with pytest.raises(ValueError, match="num_sym_faces"):
        ops.uv_atlas(torch.zeros(1, 3, 32, 64), table, 657)
    with pytest.raises(ValueError, match="table"):
        ops.uv_atlas(torch.zeros(1, 3, 32, 64), sampler)
    with pytest.raises(ValueError, match="16 x 64"):
        ops.uv_atlas(torch.zeros(1, 3, 16, 64), table)
    bad = sampler.clone()
    bad[3, 0, 1, 0] = float("nan")
    with pytest.raises(ValueError, match="uv_sampler.*finite"):
        ops.uv_atlas_table(bad, 32, 64)
    with pytest.raises(ValueError, match="tex_size"):
        compute_uvsampler(gold["verts"], gold["faces"], tex_size=1)


def test_sampler_buffer_follows_the_module(gold):
    """The sampler is a buffer outside the state dict (the reference keeps a plain attribute, so its checkpoints hold no
    such key); a deep copy keeps working and owns its own table cache."""
    import copy
    from acfm_video_3d_reconstruction_amd.texture import UVAtlasSampler
    m = UVAtlasSampler(torch.from_numpy(gold["sampler_t2"]), symmetric=True, num_sym_faces=624)
    assert m.state_dict() == {}
    x = torch.from_numpy(gold["uvimage"])
    a = m(x)
    assert len(m._tables) == 1 and m.table(x.device, 32, 64) is m.table(x.device, 32, 64)
    m2 = copy.deepcopy(m)
    assert torch.equal(m2(x), a) and m2._tables is not m._tables
