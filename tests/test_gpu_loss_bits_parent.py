"""GPU: ops.tex_mse and ops.mask_losses give, bit for bit, the sums that the build before "read only where the mask is
not zero" gave (tests/golden/loss_sums_parent.npz, recorded by tools/record_loss_parent.py with that build's
library).  The one-launch forms add their partial sums in a fixed order, so equal bits are the claim, not a tolerance."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_loss_parent as R  # noqa: E402


@pytest.mark.parametrize("i", range(len(R.CASES)))
def test_loss_sums_bit_equal_to_the_parent_build(i):
    g = np.load(os.path.join(ROOT, "tests", "golden", "loss_sums_parent.npz"))
    tex, ml = R.run_case(i, R.CASES[i])
    assert tex.dtype == np.float32 and ml.shape == (R.CASES[i][0], 4)
    assert (tex > 0).all() and (ml[:, 3] > 0).all()          # every mesh has pixels under its masks
    assert np.array_equal(tex.view(np.uint32), g["tex_%d" % i].view(np.uint32))
    assert np.array_equal(ml.view(np.uint32), g["ml_%d" % i].view(np.uint32))
