#!/usr/bin/env python3
"""Write tests/golden/boundary_subset_recorded_from_subset_host.npz: subsets and keys as boundary_sampling.subset_host /
slot_keys give them today, for the cases of tests/test_boundary_sampler.py (PIN_CASES).  A stability pin -- it records
what the host restatement computes, it does not check it.  Needs no GPU.

    python tools/record_boundary_subset.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from acfm_video_3d_reconstruction_amd.boundary_sampling import slot_keys, subset_host  # noqa: E402
from test_boundary_sampler import PIN, PIN_CASES  # noqa: E402

out = {}
for j, (seed, draw, row, P, n) in enumerate(PIN_CASES):
    out["subset_%d" % j] = subset_host(seed, draw, row, P, n)
    out["keys_%d" % j] = slot_keys(seed, draw, row, 8)
np.savez_compressed(PIN, **out)
print("wrote %s (%d bytes)" % (PIN, os.path.getsize(PIN)))
