"""The perceptual texture loss restated literally from torch ops (the spec of DESIGN.md, "Perceptual texture loss",
steps 1-5), on tensors of any one dtype and device: the float64 evaluation is the reference of tests/test_lpips.py and
tests/test_gpu_lpips.py, the float32 evaluation their yardstick.  Not a test module."""
import torch
import torch.nn.functional as F

SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
CONVS = ((0, 11, 4, 2), (3, 5, 1, 2), (6, 3, 1, 1), (8, 3, 1, 1), (10, 3, 1, 1))   # (features index, kernel, stride, pad)
CHANNELS = (64, 192, 384, 256, 256)


def lit_input(img, mask):
    """Step 1.  img [N,3,H,W], mask [N,H,W]."""
    x = 2 * (img * mask[:, None]) - 1
    return (x - x.new_tensor(SHIFT)[None, :, None, None]) / x.new_tensor(SCALE)[None, :, None, None]


def lit_taps(x, sd):
    """Step 2: the five maps after the ReLUs; sd = torchvision-named state dict, cast to x's dtype."""
    taps = []
    for idx, k, s, p in CONVS:
        if idx in (3, 6):
            x = F.max_pool2d(x, 3, 2)
        x = F.relu(F.conv2d(x, sd["features.%d.weight" % idx].to(x), sd["features.%d.bias" % idx].to(x), stride=s,
                            padding=p))
        taps.append(x)
    return taps


def lit_normalize(x, eps=1e-10):
    return x / (torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True)) + eps)


def lit_layer(a, b, lin=None):
    """Step 3.  a, b [N,C,h,w] -> [N,1,h,w]."""
    diff = (lit_normalize(a) - lit_normalize(b)) ** 2
    if lin is not None:
        diff = diff * lin.to(diff).reshape(1, -1, 1, 1)
    return diff.sum(dim=1, keepdim=True)


def lit_map(ds, H, W):
    """Step 4: ds = [d_l [N,1,h_l,w_l]] -> [N,1,H,W]."""
    return sum(F.interpolate(d, size=(H, W), mode="bilinear", align_corners=False) for d in ds)


def lit_mean(smap, mask):
    """Step 5: [N,1,H,W], mask [N,H,W] -> [N]."""
    return (smap * mask[:, None]).mean(-2).mean(-1).squeeze(-1)


def lit_loss(img_pred, img_gt, mask, sd, lins=None):
    """Steps 1-5, per prediction [N]; every input has batch N."""
    H, W = img_pred.shape[2:]
    fa, fb = lit_taps(lit_input(img_pred, mask), sd), lit_taps(lit_input(img_gt, mask), sd)
    lins = lins or [None] * 5
    return lit_mean(lit_map([lit_layer(a, b, w) for a, b, w in zip(fa, fb, lins)], H, W), mask)


def features(shape, gen):
    """Synthetic post-ReLU features [N,C,h,w] float32 with no all-zero channel vector: relu of a normal (half the
    values are 0), and a positive constant added to channel 0."""
    x = torch.relu(torch.randn(*shape, generator=gen))
    x[:, 0] += 0.25
    return x


def check(name, ours, lit32, ref64):
    """The yardstick: ours may be at most twice as far from the float64 evaluation as the literal float32 composition
    is (the factor 2 allows for a different summation order), plus 1e-7 of the largest reference magnitude."""
    ref = ref64.detach().double().cpu()
    e_ours = float((ours.detach().double().cpu() - ref).abs().max())
    e_lit = float((lit32.detach().double().cpu() - ref).abs().max())
    top = float(ref.abs().max())
    bar = 2 * e_lit + 1e-7 * top
    print("%s: ours %.3e, literal float32 %.3e, max|ref| %.3e, bar %.3e" % (name, e_ours, e_lit, top, bar))
    assert ours.shape == ref64.shape, (name, tuple(ours.shape), tuple(ref64.shape))
    assert bool(torch.isfinite(ours).all()), name
    assert e_ours <= bar, (name, e_ours, e_lit, bar)
    return e_ours, e_lit


def alex_state(seed=0):
    """A torchvision-named AlexNet feature state dict with seeded random weights (float32), scaled like torch's
    default initialisation so that every tap stays alive."""
    g = torch.Generator().manual_seed(seed)
    sd, cin = {}, 3
    for (idx, k, _, _), cout in zip(CONVS, CHANNELS):
        bound = (1.0 / (cin * k * k)) ** 0.5
        sd["features.%d.weight" % idx] = (torch.rand(cout, cin, k, k, generator=g) * 2 - 1) * bound * 1.7
        sd["features.%d.bias" % idx] = torch.rand(cout, generator=g) * bound    # positive: no dead pixel
        cin = cout
    return sd
