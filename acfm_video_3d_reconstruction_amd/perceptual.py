"""The perceptual (LPIPS, AlexNet) half of the reference's texture loss without the third-party `lpips` package
(multiframe/nnutils/loss_utils.py:359-383, called at multiframe/main.py:647-654 and predictor.py:287-349).

    features = AlexFeatures("alexnet.pth")              # a state dict or a local file; nothing is ever fetched
    loss_fn = PerceptualTextureLoss(features)
    loss = loss_fn(img_pred, img_gt, mask_pred, mask_gt, reduce=False)      # the reference's call

The definition ("Perceptual texture loss") is restated from memory of lpips 0.1.x and could not be checked
against the package.  AlexNet's five convolutions run in torch; everything around them -- the input chain, the per-layer
normalise / difference / channel sum, the upsampling, the mask and the means -- is four kinds of HIP kernels (ops.lpips_*).
Two properties of the definition are used that lpips does not use:
  * the reference side (features of the masked image, the mask's weights) does not depend on the hypothesis: img_gt and
    mask_gt may have batch N/G, and are processed once per frame (prediction n reads reference n % (N/G));
  * bilinear upsampling is linear, so the mean of mask * sum_l upsample(d_l) is sum_l sum_p d_l[p] M_l[p] with M_l the
    adjoint upsampling of mask / (H W) (ops.lpips_mask_weights): the [N,1,H,W] maps are never formed.
LPIPSAlex is the compatibility form that does return the spatial map."""
import warnings

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops

_CONVS = ((0, 3, 64, 11, 4, 2), (3, 64, 192, 5, 1, 2), (6, 192, 384, 3, 1, 1), (8, 384, 256, 3, 1, 1),
          (10, 256, 256, 3, 1, 1))    # (index in torchvision's alexnet().features, Cin, Cout, kernel, stride, padding)
_SLICE_OF = {0: 1, 3: 2, 6: 3, 8: 4, 10: 5}   # lpips.pretrained_networks.alexnet: net.slice<K>.<index>
CHANNELS = tuple(c[2] for c in _CONVS)


def _load_state(weights):
    if isinstance(weights, (str, bytes)) or hasattr(weights, "__fspath__"):
        weights = torch.load(weights, map_location="cpu")
    if not hasattr(weights, "items"):
        raise TypeError("weights: a state dict or the path of a local file holding one expected, got %s"
                        % type(weights).__name__)
    return dict(weights)


def feature_state_dict(weights):
    """The ten tensors features.{0,3,6,8,10}.{weight,bias} out of a state dict under torchvision's names (alexnet():
    the classifier's keys are dropped) or lpips's (LPIPS(net='alex'): net.slice<K>.<J>.*; the scaling layer's and the
    lin layers' keys are dropped -- lin_weights() reads the latter).  Any other key, or a missing one, is an error."""
    sd = _load_state(weights)
    out = {}
    for k, v in sd.items():
        k = k[7:] if k.startswith("module.") else k
        if k.startswith("classifier.") or k.startswith("scaling_layer.") or k.startswith("lin"):
            continue
        if k.startswith("net.slice"):
            parts = k.split(".")
            if len(parts) != 4 or not parts[2].isdigit() or _SLICE_OF.get(int(parts[2])) != int(parts[1][5:] or 0):
                raise KeyError("unexpected key %r in an lpips-named AlexNet state dict" % k)
            k = "features.%s.%s" % (parts[2], parts[3])
        out[k] = v
    want = {"features.%d.%s" % (c[0], p) for c in _CONVS for p in ("weight", "bias")}
    if set(out) != want:
        raise KeyError("AlexNet feature weights: missing %s, unexpected %s"
                       % (sorted(want - set(out)), sorted(set(out) - want)))
    return out


def lin_weights(weights):
    """The five `lin` vectors [C_l] of an lpips state dict (lin<l>.model.1.weight [1,C_l,1,1]): LPIPS(lpips=True)."""
    sd = _load_state(weights)
    sd = {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}
    try:
        lins = [sd["lin%d.model.1.weight" % l].detach().to(torch.float32).reshape(-1) for l in range(5)]
    except KeyError as exc:
        raise KeyError("no lin weights (%s) in the state dict: they come with lpips's own checkpoint" % exc) from exc
    for w, c in zip(lins, CHANNELS):
        if w.numel() != c or bool((w < 0).any()):
            raise ValueError("lin weights must be non-negative vectors of %s channels" % (CHANNELS,))
    return lins


class AlexFeatures(nn.Module):
    """AlexNet's five convolutions, in torchvision's alexnet().features layout (parameters features.0/3/6/8/10), which
    return the five maps after each ReLU: the taps of lpips.pretrained_networks.alexnet.  The last max-pool is not
    run.  weights: a state dict or a local path (feature_state_dict() names what is accepted); None keeps torch's
    default initialisation -- RANDOM features, good for tests and timing only (`pretrained` says which).
    The parameters are frozen (lpips: requires_grad=False); gradients flow to the input."""

    def __init__(self, weights=None):
        super().__init__()
        layers = []
        for idx, cin, cout, k, s, p in _CONVS:
            while len(layers) < idx:
                layers.append(nn.MaxPool2d(kernel_size=3, stride=2) if len(layers) in (2, 5) else nn.ReLU())
            layers.append(nn.Conv2d(cin, cout, kernel_size=k, stride=s, padding=p))
        layers.append(nn.ReLU())
        self.features = nn.Sequential(*layers)
        self.pretrained = weights is not None
        if weights is not None:
            self.load_state_dict(feature_state_dict(weights), strict=True)
        else:
            warnings.warn("AlexFeatures without weights: randomly initialised convolutions, not the LPIPS metric")
        for p in self.parameters():
            p.requires_grad_(False)
        self.eval()

    @staticmethod
    def tap_sizes(H, W):
        """Sizes [(h_l, w_l)] of the five taps for an H x W input."""
        def conv(n, k, s, p):
            return (n + 2 * p - k) // s + 1
        out, h, w = [], H, W
        for idx, _, _, k, s, p in _CONVS:
            if idx in (3, 6):
                h, w = conv(h, 3, 2, 0), conv(w, 3, 2, 0)
            h, w = conv(h, k, s, p), conv(w, k, s, p)
            out.append((h, w))
        if min(min(s) for s in out) < 1:
            raise ValueError("a %d x %d image is too small for AlexNet's taps" % (H, W))
        return out

    def forward(self, x):
        taps = []
        for m in self.features:
            if isinstance(m, nn.ReLU):
                x = F.relu(x, inplace=True)    # (over the convolution's output, which nothing else reads)
                taps.append(x)
            else:
                x = m(x)
        return taps


def _check_lin(lin, device):
    if lin is None:
        return None
    lin = [w.detach().to(device=device, dtype=torch.float32).reshape(-1) for w in lin]
    if [w.numel() for w in lin] != list(CHANNELS):
        raise ValueError("lin: five vectors of %s channels expected" % (CHANNELS,))
    return lin


class LPIPSAlex(nn.Module):
    """lpips.LPIPS(net='alex', lpips=(lin is not None), spatial=True): forward(in0, in1), images in [-1, 1], returns
    the [N,1,H,W] map sum_l upsample(d_l).  The compatibility form (inspection, anything that wants the map); the
    training loss is PerceptualTextureLoss, which never forms it."""

    def __init__(self, features, lin=None):
        super().__init__()
        self.net = features
        self.lin = lin
        self.register_buffer("shift", torch.tensor(ops.LPIPS_SHIFT)[None, :, None, None])
        self.register_buffer("scale", torch.tensor(ops.LPIPS_SCALE)[None, :, None, None])

    def forward(self, in0, in1):
        H, W = in0.shape[2:]
        f0 = self.net((in0 - self.shift) / self.scale)
        f1 = self.net((in1 - self.shift) / self.scale)
        lin = _check_lin(self.lin, in0.device) or [None] * 5
        out = 0
        for a, b, w in zip(f0, f1, lin):
            d = ops.lpips_layer(a, b, w)[:, None]
            out = out + F.interpolate(d, size=(H, W), mode="bilinear", align_corners=False)
        return out


class Prepared(object):
    """What PerceptualTextureLoss.prepare leaves of the reference side: its features, the mask, the mask's weights."""

    def __init__(self, feats, mask, M):
        self.feats, self.mask, self.M = feats, mask, M


class PerceptualTextureLoss(object):
    """The reference's PerceptualTextureLoss_v2 on this package's kernels: __call__(img_pred, img_gt, mask_pred,
    mask_gt, reduce=True) -> scalar or [N], img_pred [N,3,H,W]; img_gt [N or N/G,3,H,W] and mask_gt [same batch,H,W]
    may be given once per frame for its G hypotheses.  mask_pred is unused, as in the reference.
    prepare(img_gt, mask_gt) does the reference side alone; against(prepared, img_pred) the rest: a loop whose targets
    stay constant (predictor.py:287-349) prepares once."""

    def __init__(self, features, lin=None):
        if not isinstance(features, AlexFeatures):
            features = AlexFeatures(features)
        self.features = features
        self.lin = lin

    def to(self, device):
        self.features.to(device)
        return self

    def cuda(self):
        return self.to("cuda")

    def _feats(self, img, mask):
        dev = img.device
        if next(self.features.parameters()).device != dev:
            self.features.to(dev)
        return self.features(ops.lpips_input(img, mask))

    def prepare(self, img_gt, mask_gt):
        mask = mask_gt.detach().to(torch.float32)
        if img_gt.shape[0] != mask.shape[0]:
            raise ValueError("img_gt and mask_gt must have the same batch, got %d and %d"
                             % (img_gt.shape[0], mask.shape[0]))
        if img_gt.requires_grad and torch.is_grad_enabled():
            feats = self._feats(img_gt, mask)
        else:
            with torch.no_grad():
                feats = self._feats(img_gt, mask)
        M = ops.lpips_mask_weights(mask, [f.shape[2:] for f in feats])
        return Prepared(feats, mask, M)

    def against(self, prepared, img_pred, reduce=True):
        fa = self._feats(img_pred, prepared.mask)
        d = ops.lpips_layers(fa, prepared.feats, _check_lin(self.lin, img_pred.device))
        dist = ops.lpips_masked_mean(d, prepared.M)
        return dist.mean() if reduce else dist

    def __call__(self, img_pred, img_gt, mask_pred, mask_gt, reduce=True):
        return self.against(self.prepare(img_gt, mask_gt), img_pred, reduce=reduce)
