"""GPU: with up to 32 handles ops.deform_solve and its backward give, bit for bit, what the build before "up to 128
handles" gave (tests/golden/solve_parent.npz, recorded by tools/record_solve_parent.py with that build's library).
One panel of right-hand sides is the same tiles, the same k order and the same reductions as before, so equal bits are
the claim, not a tolerance."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_solve_parent as R  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "solve_parent.npz"))


@pytest.mark.parametrize("i", range(len(R.SMALL)))
def test_small_solve_bit_equal_to_the_parent_build(golden, i):
    P, g = R.run(*R.small_inputs(i))
    assert P.dtype == np.float32 and P.shape == R.SMALL[i] and g.shape == R.SMALL[i]
    assert np.isfinite(P).all() and np.abs(g).max() > 0
    assert np.array_equal(P.view(np.uint32), golden["small_%d_P" % i].view(np.uint32))
    assert np.array_equal(g.view(np.uint32), golden["small_%d_grad" % i].view(np.uint32))


@pytest.mark.parametrize("i", range(len(R.MESHES)))
def test_mesh_solve_digest_equal_to_the_parent_build(golden, i):
    P, g = R.run(*R.mesh_inputs(i))
    assert P.dtype == np.float32 and P.shape[1] == R.MESHES[i][1] and g.shape == P.shape
    assert np.isfinite(P).all() and np.abs(g).max() > 0
    assert R.digest(P) == str(golden["mesh_%d_P_sha256" % i])
    assert R.digest(g) == str(golden["mesh_%d_grad_sha256" % i])
