"""Generates azel_cameras.npz FROM THE REFERENCE ITSELF (data only; no reference source is copied).

Run in the authoring container only (needs a checkout of the reference, read-only):

    python tests/golden/make_golden_azel.py <reference>/multiframe

It imports the reference's nnutils/mesh_net.py -- with empty stand-ins for the third-party modules that file imports at
its top and the camera classes never touch (gdist, kornia, torchvision, absl.flags, pytorch3d, scipy) -- and runs
MultiCamPredictor (mesh_net.py:356-385, the decode of --az_el_cam, main.py:442-450 / 554-566) on the CPU.  Stored:
  emb [6,5,6] f32      camera embeddings (scale, tx, ty, azimuth, elevation, cyclo-rotation): randn(seed 20240611), then
                       by hand: row [0,0] all zeros; rows [g,1] the initial embedding (zeros, column 3 = g/(G-1),
                       mesh_net.py:405-416); [1,2] and [2,2] azimuth +-3 (several turns at 360 degrees); [3,2] and
                       [4,2] e0 = -25 and -40 (a negative scale under both parameter sets)
  per parameter set P in ("doc", "flags"):
    P_params [5] f64     (scale_lr_decay, scale_bias, az, el, cyc euler range in degrees):
                         doc   = (0.1, 0.9, 360, 60, 60), the documented multiframe training command (docs/setup_video.md)
                         flags = (0.05, 1.0, 30, 60, 60), the flag defaults (main.py:81-85)
    P_f32 [6,5,7] f32    MultiCamPredictor on emb
    P_f64 [6,5,7] f64    MultiCamPredictor on emb.double()
    P_dev f64            max |P_f32 - P_f64|: the float32 evaluation error of the reference itself
"""
import os
import sys
import types

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))

REF = None
PARAMS = {"doc": (0.1, 0.9, 360., 60., 60.), "flags": (0.05, 1.0, 30., 60., 60.)}


class _Anything(types.ModuleType):
    """A module whose every attribute is a callable that accepts anything (flags.DEFINE_*, base classes, ...)."""
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return type(name, (), {"__init__": lambda self, *a, **k: None, "__call__": lambda self, *a, **k: None})


def _import_mesh_net():
    for name in ("gdist", "kornia", "torchvision", "absl", "absl.flags", "pytorch3d", "pytorch3d.structures", "scipy",
                 "scipy.spatial", "utils", "utils.geometry", "utils.mesh", "nnutils.net_blocks", "nnutils.networks"):
        if name not in sys.modules:
            sys.modules[name] = _Anything(name)
    sys.modules["absl"].flags = sys.modules["absl.flags"]
    pkg = types.ModuleType("nnutils")
    pkg.__path__ = [os.path.join(REF, "nnutils")]
    sys.modules["nnutils"] = pkg
    import importlib
    return importlib.import_module("nnutils.mesh_net")        # the reference's own module, read from REF


def main():
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "nnutils")):
        sys.exit(__doc__)
    global REF
    REF = os.path.abspath(sys.argv[1])
    mesh_net = _import_mesh_net()
    G, N = 6, 5
    emb = torch.randn(G, N, 6, generator=torch.Generator().manual_seed(20240611))
    emb[0, 0] = 0
    emb[:, 1] = 0
    emb[:, 1, 3] = torch.arange(G) / (G - 1)
    emb[1, 2, 3], emb[2, 2, 3] = 3.0, -3.0
    emb[3, 2, 0], emb[4, 2, 0] = -25.0, -40.0
    out = dict(emb=emb.numpy())
    for tag, (decay, bias, az, el, cyc) in PARAMS.items():
        pred = mesh_net.MultiCamPredictor(num_cams=G, scale_lr_decay=decay, scale_bias=bias, euler_range=[az, el, cyc])
        res = {}
        for dt in (torch.float32, torch.float64):
            e = emb.to(dt)
            with torch.no_grad():
                cam = pred(e[..., :1], e[..., 1:3], e[..., 3:])
            assert cam.dtype == dt and tuple(cam.shape) == (G, N, 7)
            res[dt] = cam.numpy()
        dev = float(np.abs(res[torch.float32].astype(np.float64) - res[torch.float64]).max())
        assert (res[torch.float64][3:5, 2, 0] < 0).all()      # the negative scales passed through
        out.update({tag + "_params": np.array([decay, bias, az, el, cyc], np.float64), tag + "_f32": res[torch.float32],
                    tag + "_f64": res[torch.float64], tag + "_dev": np.float64(dev)})
        print("%s: float32 vs float64 of the reference: %.3g" % (tag, dev))
    path = os.path.join(OUT, "azel_cameras.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
