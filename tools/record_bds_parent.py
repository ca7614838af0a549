"""Record tests/golden/bds_parent.npz: what a given build of libacfm_hip.so answers to acfm_bds_loss (every point,
the zero-fill + atomics finish) on inputs made to pin its tie rule -- the fixture
tests/test_gpu_loss_reductions.py compares later builds with, bit for bit.

    python tools/record_bds_parent.py --lib PATH/libacfm_hip.so [--out tests/golden/bds_parent.npz]

Run it with the library of the commit BEFORE a change to k_bds_loss.  It loads the library by itself (ctypes, no
package import), so any build of the 2.x ABI will do; a library that reports another acfm_version() has other argument
lists behind the same names and is refused.

The inputs: vertices and boundary points on the grid k / 16, k in [-16, 16] -- many vertices coincide and many
points are equally far from several vertices, so the answer depends on the tie rule (first nearest vertex in
ascending order) everywhere; a mesh with nothing visible and one with a single visible vertex per case.  Every
squared distance is a multiple of 2^-8 below 8 and every per-mesh sum stays below 2^24 such units, so the float
sums are exact in any order: the recorded loss does not depend on the order the old kernel's atomics arrived in.
"""
import argparse
import ctypes
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ABI_VERSION = 2000   # acfm_version() of the header the signature below is taken from
# (N, ref_batch, V, P)
CASES = [(3, 3, 37, 70), (4, 2, 642, 800), (3, 1, 2562, 1537), (2, 2, 3, 1), (3, 3, 65, 64)]


def make_case(rng, N, RB, V, P):
    """-> int8 vertex numerators [N,V,2], int8 point numerators [RB,P,2] (coordinates = numerator / 16), point flags
    [RB,P] u8, visibility [N,V] u8."""
    xy = rng.integers(-16, 17, (N, V, 2)).astype(np.int8)
    bd = rng.integers(-16, 17, (RB, P, 2)).astype(np.int8)
    flag = (rng.uniform(size=(RB, P)) > 0.15).astype(np.uint8)
    vis = (rng.uniform(size=(N, V)) > 0.45).astype(np.uint8)
    vis[N - 1] = 0                                    # nothing visible
    if N > 1:
        vis[N - 2] = 0
        vis[N - 2, V - 1] = 1                         # one visible vertex, the last one
    return xy, bd, flag, vis


def floats(xy, bd, flag):
    v = xy.astype(np.float32) / np.float32(16)
    b = np.concatenate([bd.astype(np.float32) / np.float32(16), flag[..., None].astype(np.float32)], -1)
    return v, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "bds_parent.npz"))
    a = ap.parse_args()
    lib = ctypes.CDLL(os.path.abspath(a.lib))
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.acfm_version.restype, lib.acfm_version.argtypes = ci, []
    if lib.acfm_version() != ABI_VERSION:
        raise SystemExit("%s reports acfm_version() = %d, this tool binds version %d of include/acfm_hip.h: record with "
                         "the tool of the library's own commit, or rebuild the library (make -C "
                         "acfm_video_3d_reconstruction_amd/csrc)" % (a.lib, lib.acfm_version(), ABI_VERSION))
    lib.acfm_bds_loss.restype = ci
    lib.acfm_bds_loss.argtypes = [vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, ctypes.c_size_t, vp]
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(20240)
    out = {}
    for i, (N, RB, V, P) in enumerate(CASES):
        xy, bd, flag, vis = make_case(rng, N, RB, V, P)
        v, b = floats(xy, bd, flag)
        tv, tb, tvis = torch.from_numpy(v).to(dev), torch.from_numpy(b).to(dev), torch.from_numpy(vis).to(dev)
        loss = torch.empty(N, dtype=torch.float32, device=dev)
        arg = torch.empty((N, P), dtype=torch.int32, device=dev)
        rc = lib.acfm_bds_loss(tv.data_ptr(), tb.data_ptr(), tvis.data_ptr(), None, N, V, P, RB, 0, 0, loss.data_ptr(),
                               arg.data_ptr(), None, None, 0, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        torch.cuda.synchronize()
        for k, x in (("xy", xy), ("bd", bd), ("flag", flag), ("vis", vis), ("loss", loss.cpu().numpy()),
                     ("argmin", arg.cpu().numpy())):
            out["c%d_%s" % (i, k)] = x
        out["c%d_rb" % i] = np.int32(RB)
        print("case %d N=%d RB=%d V=%d P=%d loss=%s" % (i, N, RB, V, P, loss.cpu().numpy()))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **out)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
