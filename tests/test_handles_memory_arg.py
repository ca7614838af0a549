"""CPU: the `memory` argument of handles.geodesic_distance_matrix / geodesic_lbs_logits on the host path.  Arrays and
host tensors never reach a GPU kernel, so the argument changes nothing there -- but it is validated."""
import numpy as np
import pytest
import torch

import handles_meshes as HM
from acfm_video_3d_reconstruction_amd import handles

MEMORY = ("lds", "device", "auto")


@pytest.fixture(scope="module")
def prism():
    v, f = HM.jittered_prism()
    return v, f, handles.geodesic_distance_matrix(v, f, 3), handles.geodesic_lbs_logits(v, f, 4, steiner=3)


@pytest.mark.parametrize("memory", MEMORY)
def test_distance_matrix_ignores_memory_on_arrays(prism, memory):
    v, f, D, _ = prism
    assert np.array_equal(handles.geodesic_distance_matrix(v, f, 3, memory=memory), D)
    got = handles.geodesic_distance_matrix(torch.from_numpy(v), torch.from_numpy(f), 3, [5, 0], memory=memory)
    assert torch.is_tensor(got) and np.array_equal(got.numpy(), D[[5, 0]])


@pytest.mark.parametrize("memory", MEMORY)
def test_lbs_logits_ignore_memory_on_arrays(prism, memory):
    v, f, _, (logits, idx) = prism
    got, got_idx = handles.geodesic_lbs_logits(v, f, 4, steiner=3, memory=memory)
    assert got_idx.tolist() == idx.tolist() and np.array_equal(got, logits)


@pytest.mark.parametrize("bad", ("global", "LDS", None, 0))
def test_unknown_memory_is_refused(prism, bad):
    v, f = prism[:2]
    for call in (lambda: handles.geodesic_distance_matrix(v, f, 3, memory=bad),
                 lambda: handles.geodesic_lbs_logits(v, f, 4, steiner=3, memory=bad)):
        with pytest.raises(ValueError) as e:
            call()
        assert all('"%s"' % name in str(e.value) for name in MEMORY)
