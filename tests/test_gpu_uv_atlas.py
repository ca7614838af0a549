"""GPU: ops.uv_atlas (csrc/acfm_uvatlas.hip) and texture.UVAtlasSampler against the lines of mesh_net.py:169-179
evaluated in float64 on the CPU, on the same float32-rounded inputs, gradients by autograd.

Bars.  float32 cannot meet 1e-6 here: x = (u + 1) / 2 * (Wu - 1) carries an ulp of 1.5e-5 pixel at Wu = 256, times the
image slope.  So every case also evaluates the same lines in torch-CPU float32 and measures THAT error against float64;
the GPU's error may be at most twice it (two float32 evaluations of one formula, differing in operation order and
tanhf), with floors of 2e-6 absolute forward (a handful of roundings of values <= 1) and 1e-6 of max|grad| for the
gradient -- and, as a condition, no forward bar above 1e-4 and no gradient bar above 1e-4 of max|grad|.  UV images are
drawn from N(0, 1).  Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from conftest import load_golden

pytestmark = pytest.mark.gpu


def _d():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _lines(uvimage, sampler, nsym):
    """mesh_net.py:169-179 on tensors of one dtype and device (sampler [F',T,T,2])."""
    Fp, T, B = sampler.shape[0], sampler.shape[1], uvimage.shape[0]
    tex = TF.grid_sample(uvimage, sampler.reshape(1, Fp, T * T, 2).repeat(B, 1, 1, 1), align_corners=True)
    tex = tex.reshape(B, -1, Fp, T, T).permute(0, 2, 3, 4, 1)
    tex = (torch.tanh(tex) + 1) / 2
    return torch.cat([tex, tex[:, -nsym:]], 1) if nsym else tex


class Case:
    """One configuration: inputs, the float64 reference, the torch-CPU float32 evaluation, the bars, the GPU's run."""

    def __init__(self, tag, uvimage, sampler, nsym, grad=None, seed=0):
        from acfm_video_3d_reconstruction_amd import ops
        self.tag, self.nsym = tag, int(nsym)
        self.uvimage = uvimage.to(torch.float32).contiguous()
        self.sampler = sampler.to(torch.float32).contiguous()            # the float32-rounded inputs of every evaluation
        B, Fp, T = uvimage.shape[0], sampler.shape[0], sampler.shape[1]
        if grad is None:
            grad = torch.randn(B, Fp + self.nsym, T, T, 3, generator=torch.Generator().manual_seed(1000 + seed))
        self.grad = grad.to(torch.float32)
        ev = {}
        for dt in (torch.float64, torch.float32):
            x = self.uvimage.to(dt).clone().requires_grad_(True)   # (a copy: .to(float32) is self.uvimage itself)
            a = _lines(x, self.sampler.to(dt), self.nsym)
            ev[dt] = (a.detach(), torch.autograd.grad(a, x, self.grad.to(dt))[0])
        self.atlas64, self.gx64 = ev[torch.float64]
        self.scale = float(self.gx64.abs().max())
        self.cpu_fwd = float((ev[torch.float32][0].double() - self.atlas64).abs().max())
        self.cpu_grad = float((ev[torch.float32][1].double() - self.gx64).abs().max())
        self.fwd_bar = max(2 * self.cpu_fwd, 2e-6)
        self.grad_bar = max(2 * self.cpu_grad, 1e-6 * self.scale)
        print("%s: torch-CPU float32 vs float64: forward %.3e, gradient %.3e (%.3e of max|grad| = %.3e); bars %.3e / %.3e"
              % (tag, self.cpu_fwd, self.cpu_grad, self.cpu_grad / max(self.scale, 1e-300), self.scale, self.fwd_bar,
                 self.grad_bar))
        assert self.fwd_bar <= 1e-4 and self.grad_bar <= 1e-4 * self.scale      # the caps: conditions of the comparison
        d = _d()
        self.table = ops.uv_atlas_table(self.sampler.to(d), uvimage.shape[2], uvimage.shape[3])
        self.atlas, self.gx = self.run(self.grad)

    def run(self, grad):
        from acfm_video_3d_reconstruction_amd import ops
        x = self.uvimage.to(_d()).requires_grad_(True)
        a = ops.uv_atlas(x, self.table, self.nsym)
        gx, = torch.autograd.grad(a, x, grad.to(_d()))
        return a.detach(), gx

    def check(self):
        a, gx = self.atlas.cpu(), self.gx.cpu()
        assert a.shape == self.atlas64.shape and gx.shape == self.gx64.shape
        ef = float((a.double() - self.atlas64).abs().max())
        eg = float((gx.double() - self.gx64).abs().max())
        print("%s: GPU vs float64: forward %.3e (bar %.3e), gradient %.3e = %.3e of max|grad| (bar %.3e)"
              % (self.tag, ef, self.fwd_bar, eg, eg / max(self.scale, 1e-300), self.grad_bar))
        assert not torch.isnan(a).any() and not torch.isnan(gx).any()
        assert ef <= self.fwd_bar
        assert eg <= self.grad_bar
        return self


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@pytest.fixture(scope="module")
def gold():
    return load_golden("uv_atlas")


@pytest.fixture(scope="module")
def case1(gold):
    """The reference's configuration: the golden symmetric sampler, T = 6, 128 x 256, B = 2, S = 624."""
    return Case("case 1 (T=6, 128x256, B=2, S=624)", _randn(2, 3, 128, 256, seed=1),
                torch.from_numpy(gold["sampler_t6"]), int(gold["num_sym_faces"]), seed=1)


def test_reference_configuration(case1):
    case1.check()
    assert tuple(case1.atlas.shape) == (2, 1280, 6, 6, 3)


def test_tex_size_2(gold):
    Case("case 2a (T=2, 32x64, B=3, S=624)", _randn(3, 3, 32, 64, seed=2), torch.from_numpy(gold["sampler_t2"]),
         int(gold["num_sym_faces"]), seed=2).check()


def test_non_symmetric_1280_faces(gold):
    from acfm_video_3d_reconstruction_amd import texture
    sampler = texture.compute_uvsampler(gold["verts"], gold["faces"], tex_size=6)
    assert sampler.shape == (1280, 6, 6, 2)
    Case("case 2b (1280 faces, T=6, 128x256, B=1, nsym=0)", _randn(1, 3, 128, 256, seed=3), torch.from_numpy(sampler), 0,
         seed=3).check()


@pytest.mark.parametrize("S", [5, 1])
def test_odd_everything(S):
    sampler = torch.rand(5, 3, 3, 2, generator=torch.Generator().manual_seed(4)) * 2 - 1
    Case("case 3 (F'=5, T=3, 5x7, B=3, S=%d)" % S, _randn(3, 3, 5, 7, seed=5), sampler, S, seed=6).check()


def test_borders():
    """Samples exactly on +-1 of either axis, samples just past the border (some taps outside) and samples far outside
    (all taps outside: exactly 0.5, and no gradient leaves them)."""
    on = [(1, 0.3), (-1, -0.2), (0.1, 1), (0.4, -1), (1, 1), (-1, -1), (1, -1), (-1, 1)]
    past = [(1.1, 0.0), (-1.15, 0.3), (0.2, 1.2), (0.3, -1.05), (1.07, -1.13), (-1.2, 1.2), (1.2, 0.5), (-0.6, -1.2)]
    out = [(3, 3), (-3, 0.1), (0.2, -3), (3, -3)]
    inner = (torch.rand(4, 2, generator=torch.Generator().manual_seed(7)) * 2 - 1).tolist()
    sampler = torch.tensor(on + past + out + inner, dtype=torch.float32).reshape(6, 2, 2, 2)
    img = _randn(2, 3, 6, 9, seed=8)
    c = Case("case 4 (borders, 6x9, B=2, S=2)", img, sampler, 2, seed=9).check()
    flat = c.atlas[:, :6].reshape(2, 24, 3)
    assert torch.equal(flat[:, 16:20], torch.full((2, 4, 3), 0.5, device=flat.device))
    assert float((flat[:, :16] - 0.5).abs().min()) > 0                     # (every other sample does take a tap)
    # a gradient that arrives at the far-outside texels alone goes nowhere
    g = torch.zeros(2, 8, 2, 2, 3)
    g[:, 4] = _randn(2, 2, 2, 3, seed=10)                                    # face 4 = samples 16..19
    assert torch.equal(c.run(g)[1], torch.zeros(2, 3, 6, 9, device=_d()))
    # the taps of a sample on the last column / row: the partner past the border is "outside"
    taps = c.table.pix_taps.cpu().tolist()
    assert 0 < len(taps) < 4 * 24


def _pile(Fp, T, H, W, B, tag, seed, nsym=0):
    """Every sample at one interior point: four pixels carry Fp*T*T entries each."""
    sampler = torch.tensor([0.3, -0.45]).repeat(Fp, T, T, 1)
    c = Case(tag, _randn(B, 3, H, W, seed=seed), sampler, nsym, seed=seed + 1).check()
    start = c.table.pix_start.cpu()
    lens = (start[1:] - start[:-1]).reshape(H, W)
    x, y = int(0.65 * (W - 1)), int(0.275 * (H - 1))
    want = torch.zeros(H, W, dtype=lens.dtype)
    want[y:y + 2, x:x + 2] = Fp * T * T
    assert torch.equal(lens, want)
    gx = c.gx.cpu()
    assert not torch.isnan(gx).any()
    assert torch.equal(gx[:, :, want == 0], torch.zeros(B, 3, H * W - 4))     # exactly 0.0 elsewhere
    assert float(gx[:, :, want > 0].abs().min()) > 0
    return c


def test_pile_up():
    _pile(64, 6, 9, 9, 2, "case 5 (pile-up: 2304 entries on four pixels of 9x9, B=2)", 11)


@pytest.mark.parametrize("Fp,T", [(8, 2), (33, 1), (16, 2)])
def test_list_lengths_around_the_wave_threshold(Fp, T):
    """Lists of 32 entries are walked by one lane, of 33 and more by the whole wave (UV_SERIAL of the kernel): both
    sides of the threshold, and one list of exactly a wave's width."""
    _pile(Fp, T, 5, 5, 3, "lists of %d entries (5x5, B=3)" % (Fp * T * T), 20 + Fp, nsym=Fp // 2)


def test_untouched_pixels_are_exactly_zero(case1):
    start = case1.table.pix_start.cpu()
    empty = (start[1:] == start[:-1]).reshape(128, 256)
    print("case 1: %d of %d pixels have no tap, longest list %d, %d entries"
          % (int(empty.sum()), empty.numel(), int((start[1:] - start[:-1]).max()), int(start[-1])))
    assert int(empty.sum()) > 0 and int(start[-1]) == case1.table.pix_taps.numel()
    gx = case1.gx.cpu()
    assert torch.equal(gx[:, :, empty], torch.zeros(2, 3, int(empty.sum())))
    assert float(gx[:, :, ~empty].abs().max()) > 0


def test_mirroring(case1):
    Fp, S = 656, 624
    a = case1.atlas
    assert torch.equal(a[:, Fp:], a[:, Fp - S:Fp])
    vals = _randn(2, S, 6, 6, 3, seed=12)
    on_mirror = torch.zeros(2, Fp + S, 6, 6, 3)
    on_mirror[:, Fp:] = vals
    on_source = torch.zeros(2, Fp + S, 6, 6, 3)
    on_source[:, Fp - S:Fp] = vals
    gm, gs = case1.run(on_mirror)[1], case1.run(on_source)[1]
    assert float(gm.abs().max()) > 0 and torch.equal(gm, gs)


def test_reproducible(case1):
    for _ in range(2):
        a, gx = case1.run(case1.grad)
        assert torch.equal(a, case1.atlas) and torch.equal(gx, case1.gx)


def test_saturation(gold):
    """Entries +-20 (the sign constant over quarters of the image, so that most texels saturate and the texels that
    straddle a sign change do not): a texel whose float64 pre-activation is past +-15 is exactly 0 or 1."""
    sign = torch.ones(2, 3, 32, 64)
    sign[:, :, :, 32:] = -1
    sign[1, :, 16:] *= -1
    sign[:, 1] *= -1
    sampler = torch.from_numpy(gold["sampler_t2"]).float()
    c = Case("case 9 (+-20, T=2, 32x64, B=2, S=624)", 20 * sign, sampler, 624, seed=13).check()
    pre = TF.grid_sample((20 * sign).double(), sampler.double().reshape(1, 656, 4, 2).repeat(2, 1, 1, 1),
                         align_corners=True).reshape(2, 3, 656, 2, 2).permute(0, 2, 3, 4, 1)
    a = c.atlas.cpu()[:, :656]
    hi, lo = pre >= 15, pre <= -15
    print("case 9: %d texel values saturate high, %d low, %d do not" % (int(hi.sum()), int(lo.sum()), int((~hi & ~lo).sum())))
    assert int(hi.sum()) > 1000 and int(lo.sum()) > 1000 and int((~hi & ~lo).sum()) > 10
    assert bool((a[hi] == 1.0).all()) and bool((a[lo] == 0.0).all())
    assert bool(torch.isfinite(c.gx).all()) and c.scale > 0


def test_whole_chain(gold, case1):
    """UV image -> atlas -> texture render of N = 4 meshes sharing B = 2 atlases (G = 2) + the texture-cycle term, and
    back: the operator against the torch composition on the GPU in its place, same renderer."""
    from acfm_video_3d_reconstruction_amd import ops
    from acfm_video_3d_reconstruction_amd.nnutils.nmr import NeuralRenderer
    from acfm_video_3d_reconstruction_amd.synthetic import batch_verts, make_cams
    from acfm_video_3d_reconstruction_amd.texture import UVAtlasSampler
    d = _d()
    rng = np.random.default_rng(14)
    N, H = 4, 32
    tv = torch.tensor(batch_verts(gold["verts"].astype(np.float32), N, rng), device=d)
    tc = torch.tensor(make_cams(N, rng), device=d)
    faces = torch.from_numpy(gold["faces"])[None].repeat(N, 1, 1).to(d)
    sampler = case1.sampler.to(d)
    head = UVAtlasSampler(sampler, symmetric=True, num_sym_faces=624).to(d)
    w = _randn(N, 3, H, H, seed=15).to(d)
    r = NeuralRenderer(H)

    def chain(to_atlas):
        x = case1.uvimage.detach().to(d).requires_grad_(True)
        atlas = to_atlas(x)
        img, sil, _ = r(tv, faces, tc, textures=atlas)
        ((img * w).sum() + ops.texture_cycle(atlas, 2)).backward()
        return img.detach(), sil.detach(), x.grad, atlas.detach()

    img, sil, gx, atlas = chain(head)
    img_t, sil_t, gx_t, atlas_t = chain(lambda x: _lines(x, sampler, 624).contiguous())
    scale = float(gx_t.abs().max())
    bar = case1.grad_bar / case1.scale * scale
    err = float((gx - gx_t).abs().max())
    ndiff = int((atlas != atlas_t).sum())
    print("whole chain: covered %.3f; atlases differ in %d of %d values (max %.3e); renders differ in %d values; "
          "|grad - grad_torch| max %.3e = %.3e of max|grad| %.3e (bar %.3e)"
          % (float((sil > 0.5).float().mean()), ndiff, atlas.numel(), float((atlas - atlas_t).abs().max()),
             int((img != img_t).sum()), err, err / scale, scale, bar))
    assert float((sil > 0.5).float().mean()) > 0.1 and scale > 0
    assert err <= bar
    assert torch.equal(img, img_t)


def test_capture(gold):
    from acfm_video_3d_reconstruction_amd.texture import UVAtlasSampler
    d = _d()
    sampler = torch.from_numpy(gold["sampler_t2"])
    head = UVAtlasSampler(sampler, symmetric=True, num_sym_faces=624).to(d)
    x = _randn(2, 3, 32, 64, seed=16).to(d).requires_grad_(True)
    go = _randn(2, 1280, 2, 2, 3, seed=17).to(d)

    def step():
        a = head(x)
        return a, torch.autograd.grad(a, x, go)[0]

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()                                   # (the first run builds the table, eagerly)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = step()
    with torch.no_grad():
        x.copy_(_randn(2, 3, 32, 64, seed=18).to(d))
    g.replay()
    torch.cuda.synchronize()
    got = [t.detach().clone() for t in outs]
    ref = step()
    assert float(got[1].abs().max()) > 0
    assert torch.equal(got[0], ref[0].detach()) and torch.equal(got[1], ref[1])


def test_capture_with_an_unbuilt_table_raises(gold):
    from acfm_video_3d_reconstruction_amd.texture import UVAtlasSampler
    d = _d()
    head = UVAtlasSampler(torch.from_numpy(gold["sampler_t2"])).to(d)       # never run: no table for this device yet
    x = torch.zeros(1, 3, 32, 64, device=d)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="uv_atlas_table"):
        with torch.cuda.graph(g):
            y = x + 1.0                       # (so that the abandoned capture is not an empty graph)
            head(y)
    torch.cuda.synchronize()
    assert tuple(head(x).shape) == (1, 656, 2, 2, 3)                         # eager: builds the table and runs


def test_module_follows_its_device_and_data_parallel(gold):
    """.to() moves the sampler buffer, the table is cached per device, and two DataParallel replicas on this card share
    the cache of the module they were made from."""
    from acfm_video_3d_reconstruction_amd.texture import UVAtlasSampler
    d = _d()
    head = UVAtlasSampler(torch.from_numpy(gold["sampler_t2"]), symmetric=True, num_sym_faces=624)
    assert not head.uv_sampler.is_cuda
    head = head.to(d)
    assert head.uv_sampler.is_cuda
    x = _randn(4, 3, 32, 64, seed=19).to(d)
    want = head(x)
    dp = torch.nn.DataParallel(head, device_ids=[0, 0])
    for _ in range(2):
        assert torch.equal(dp(x), want)
    assert len(head._tables) == 1
