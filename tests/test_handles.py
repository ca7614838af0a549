"""CPU: handles.py -- the edge-Steiner distances (host path, scipy in float64) against analytic geodesics, the
farthest-point sampling of mesh_net.py:54-85 and the lbs logits of mesh_net.py:523-544.

Bars.  The Steiner distance is an upper bound of the exact geodesic that can only fall when the points of one graph
are among those of the next (m -> m' with (m' + 1) % (m + 1) == 0: the chain 0, 1, 3, 7, 15).  Its maximum relative
error at m = 15 was measured on exactly these meshes with scipy's Dijkstra when the definition was fixed: 7.6e-4 on the
flat meshes, 2.0e-3 on the prism; the caps 1.2e-3 and 3e-3 are 1.5 x that -- a property of the graph, not of an
implementation."""
import numpy as np
import pytest
import torch

import handles_meshes as HM

CHAIN = (0, 1, 3, 7, 15)


@pytest.fixture(scope="module")
def chains():
    """{mesh: (exact, {m: D})}: every distance matrix once."""
    from acfm_video_3d_reconstruction_amd import handles
    out = {}
    for name, (make, exact) in HM.KNOWN.items():
        v, f = make()
        out[name] = (v, f, exact(v), {m: handles.geodesic_distance_matrix(v, f, m) for m in CHAIN})
    return out


@pytest.mark.parametrize("name", sorted(HM.KNOWN))
def test_upper_bound_nested_chain_and_error(chains, name):
    v, f, exact, D = chains[name]
    off = ~np.eye(v.shape[0], dtype=bool)
    prev = None
    for m in CHAIN:
        assert D[m].shape == exact.shape and D[m].dtype == np.float64
        assert np.all(np.diag(D[m]) == 0)
        err = float(((D[m] - exact)[off] / exact[off]).max())
        print("%s m=%d: max relative error %.3e, min(D - exact) %.3e" % (name, m, err, (D[m] - exact).min()))
        assert np.all(D[m] >= exact - 1e-12)
        if prev is not None:
            assert np.all(D[m] <= prev + 1e-12)
        prev = D[m]
    cap = 3e-3 if name == "prism" else 1.2e-3
    assert float(((D[15] - exact)[off] / exact[off]).max()) <= cap


@pytest.mark.parametrize("name", sorted(HM.KNOWN))
def test_m0_is_dijkstra_on_the_edge_graph(chains, name):
    v, f, _, D = chains[name]
    ref = HM.edge_graph_dijkstra(v, f)
    assert np.abs(D[0] - ref).max() <= 1e-12


def test_u_strip_tips_are_near_in_space_and_far_on_the_surface():
    from acfm_video_3d_reconstruction_amd import handles
    v, f = HM.u_strip()
    D = handles.geodesic_distance_matrix(v, f, 15, sources=[0])
    euclid = np.linalg.norm(v[0] - v[18])
    print("U-strip tips: geodesic %.4f, Euclidean %.4f" % (D[0, 18], euclid))
    assert euclid == 1.0 and abs(D[0, 18] - 9.0) <= 1e-9      # same row of the strip: the straight unfolded line
    assert D[0, 18] > 2 * euclid
    assert D[0, 19] > 2 * np.linalg.norm(v[0] - v[19])


def test_tensors_sources_and_types():
    from acfm_video_3d_reconstruction_amd import handles
    v, f = HM.prism()
    D = handles.geodesic_distance_matrix(v, f, 3)
    Dt = handles.geodesic_distance_matrix(torch.from_numpy(v), torch.from_numpy(f), 3, sources=torch.tensor([5, 2, 5]))
    assert torch.is_tensor(Dt) and Dt.dtype == torch.float64 and tuple(Dt.shape) == (3, v.shape[0])
    assert np.array_equal(Dt.numpy(), D[[5, 2, 5]])


def test_farthest_point_sampling_first_maximum_wins():
    from acfm_video_3d_reconstruction_amd.handles import farthest_point_sampling
    D = np.array([[0, 1, 4, 4, 2],
                  [1, 0, 3, 3, 1],
                  [4, 3, 0, 2, 5],
                  [4, 3, 2, 0, 5],
                  [2, 1, 5, 5, 0]], np.float64)
    # far = D[0] = (0,1,4,4,2): the tie 2 / 3 goes to 2; min with D[2] = (0,1,0,2,2): the tie 3 / 4 goes to 3;
    # min with D[3] = (0,1,0,0,2) -> 4; then (0,1,0,0,0) -> 1
    idx = farthest_point_sampling(D, 4)
    assert idx.dtype == np.int64 and idx.tolist() == [0, 2, 3, 4, 1]
    assert farthest_point_sampling(D, 2).tolist() == [0, 2, 3]                    # start = 0, length num + 1
    assert farthest_point_sampling(torch.from_numpy(D), 1, start=4).tolist() == [4, 2]
    assert farthest_point_sampling(D, 0).tolist() == [0]


def _lbs_literal(D, idx_pts, pp=16):
    """mesh_net.py:529-542, line for line, on a given distance matrix."""
    dists_full = torch.zeros(D.shape[0], len(idx_pts)).float()
    for i in range(D.shape[0]):
        dists_full[i] = torch.from_numpy(D[i, idx_pts])
    lbs = 1 / dists_full ** pp
    lbs[torch.isinf(lbs)] = 0
    max_lbs = lbs.max(dim=0)[0]
    for i_lbs, idx_pt in enumerate(idx_pts):
        lbs[idx_pt, i_lbs] = max_lbs[i_lbs]
    return torch.log(torch.clamp(lbs, min=0.0000000001))


def test_lbs_logits_against_the_reference_lines():
    from acfm_video_3d_reconstruction_amd import handles
    v, f = HM.prism()
    D = handles.geodesic_distance_matrix(v, f, 3)
    idx = np.array([0, 9, 17, 24])
    D[9, 0] = D[0, 9] = 100.0       # 1 / d^16 = 1e-32: below the floor
    D[3, 17] = 0.0                  # a distance of 0 off the handle row: 1 / 0 = inf -> 0 -> the floor
    got = handles.lbs_logits_from_distances(D, idx)
    ref = _lbs_literal(D, idx)
    assert tuple(got.shape) == (v.shape[0], 4) and got.dtype == torch.float32
    assert torch.equal(got, ref)
    floor = float(torch.log(torch.tensor(1e-10)))
    assert float(got.min()) == floor and float(got[9, 0]) == floor and float(got[3, 2]) == floor
    for i, p in enumerate(idx):
        assert float(got[p, i]) == float(got[:, i].max())


def test_geodesic_lbs_logits_end_to_end():
    from acfm_video_3d_reconstruction_amd import handles
    v, f = HM.prism()
    logits, idx = handles.geodesic_lbs_logits(v, f, 6, steiner=3)
    D = handles.geodesic_distance_matrix(v, f, 3)
    want = np.sort(handles.farthest_point_sampling(D, 5))
    assert isinstance(logits, np.ndarray) and logits.dtype == np.float32 and logits.shape == (v.shape[0], 6)
    assert idx.tolist() == want.tolist() and idx[0] == 0 and len(idx) == 6
    assert np.array_equal(logits, _lbs_literal(D, idx).numpy())
    lt, it = handles.geodesic_lbs_logits(torch.from_numpy(v), torch.from_numpy(f), 6, steiner=3)
    assert torch.is_tensor(lt) and np.array_equal(lt.numpy(), logits) and it.tolist() == idx.tolist()


def test_refusals():
    from acfm_video_3d_reconstruction_amd import handles
    v, f = HM.square()
    with pytest.raises(ValueError, match="steiner"):
        handles.geodesic_distance_matrix(v, f, 21)
    with pytest.raises(ValueError, match="steiner"):
        handles.geodesic_distance_matrix(v, f, -1)
    bad = f.copy()
    bad[3, 1] = v.shape[0]
    with pytest.raises(ValueError, match="vertex ids"):
        handles.geodesic_distance_matrix(v, bad, 1)
    bad[3, 1] = -1
    with pytest.raises(ValueError, match="vertex ids"):
        handles.geodesic_distance_matrix(v, bad, 1)
    # two components: the distances are +inf across, and the logits refuse
    v2 = np.concatenate([v, v + np.array([10.0, 0, 0])], 0)
    f2 = np.concatenate([f, f + v.shape[0]], 0)
    D = handles.geodesic_distance_matrix(v2, f2, 1)
    n = v.shape[0]
    assert np.isinf(D[:n, n:]).all() and np.isinf(D[n:, :n]).all() and np.isfinite(D[:n, :n]).all()
    with pytest.raises(ValueError, match="not connected"):
        handles.geodesic_lbs_logits(v2, f2, 4, steiner=1)


def test_ops_refuses_host_tensors():
    from acfm_video_3d_reconstruction_amd import ops
    v, f = HM.square()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.geodesic_distances(torch.from_numpy(v).float(), torch.from_numpy(f))
