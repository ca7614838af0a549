"""Generates symmetric_template.npz FROM THE REFERENCE ITSELF (data only; no reference source is copied).

Run in the authoring container only (needs /root/reference, read-only):

    python tests/golden/make_golden_symmetric.py

It imports the reference's utils/mesh.py (after restoring the ``np.float`` alias numpy 2 dropped, which that file still
uses) and stores, for every subdivision level L in `levels` (1, 2, 3, and 4 while the file stays smaller than the
largest .npz already beside it):
  raw_verts_L [V,3] f64, raw_faces_L [F,3] i64      create_sphere(L)
  verts_L [V,3] f64, faces_L [F,3] i64, counts_L [4] i64 = (num_indept, num_sym, num_indept_faces, num_sym_faces)
                                                    make_symmetric(create_sphere(L))
"""
import glob
import os
import sys

import numpy as np

REF = "/root/reference/multiframe"
OUT = os.path.dirname(os.path.abspath(__file__))
NAME = "symmetric_template.npz"

np.float = float
sys.path.insert(0, REF)
from utils import mesh as ref_mesh  # noqa: E402  (the reference's own module)


def level(L):
    rv, rf = ref_mesh.create_sphere(L)
    rv, rf = np.array(rv, np.float64), np.array(rf, np.int64)
    v, f, n_indept, n_sym, nf_indept, nf_sym = ref_mesh.make_symmetric(rv.copy(), rf.copy())
    return {"raw_verts_%d" % L: rv, "raw_faces_%d" % L: rf, "verts_%d" % L: np.asarray(v, np.float64),
            "faces_%d" % L: np.asarray(f, np.int64),
            "counts_%d" % L: np.array([n_indept, n_sym, nf_indept, nf_sym], np.int64)}


def main():
    path = os.path.join(OUT, NAME)
    limit = max(os.path.getsize(p) for p in glob.glob(os.path.join(OUT, "*.npz")) if os.path.basename(p) != NAME)
    data = {}
    for L in (1, 2, 3):
        data.update(level(L))
    with_4 = dict(data)
    with_4.update(level(4))
    np.savez_compressed(path, levels=np.array([1, 2, 3, 4], np.int64), **with_4)
    if os.path.getsize(path) >= limit:
        np.savez_compressed(path, levels=np.array([1, 2, 3], np.int64), **data)
    print("%s: %d bytes (largest other .npz: %d), levels %s" % (path, os.path.getsize(path), limit,
                                                                np.load(path)["levels"].tolist()))


if __name__ == "__main__":
    main()
