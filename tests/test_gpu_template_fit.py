"""The template-fit kernels of csrc/acfm_fit.hip on the GPU -- chamfer (k_chamfer, k_chamfer_bwd and its global pair
k_chamfer_bwd_own / k_chamfer_bwd_scatter), edge length (k_edge_len / _bwd), normal consistency (k_normal_cons / _bwd)
-- through the shim's public functions, against the float64 helpers of tests/test_shim_template_fit.py, whose CPU tests
put every input used here through the float32 host path first.  Bars: see that file's docstring; every measured figure
is printed before it is asserted.

The sizes at which the chamfer kernels change path, each with a case either side (the other cloud at 64 points):
  * 64 query points per workgroup (63 x 65, 64 x 64);
  * 1024 candidates per round -- four waves x a 256-point LDS tile: 1024 / 1025 candidates, in both directions;
  * the backward's LDS: 12 B per point, 5462 points (the first size past 64 KB), 12800 (150 KB, the bound) and 12801
    points on either side (the global-atomic kernels)."""
import numpy as np
import pytest
import torch

from test_shim_template_fit import (BOUND_PAIRS, CH_BWD_LDS_MAX_P, CH_ROUND, EDGE_RUNS, LDS_64K_P, NORMAL_RUNS, SIZE_PAIRS,
                                    chamfer_case, chamfer_host, chamfer_reference, check_chamfer, check_mesh_term,
                                    mesh_case, run_chamfer, run_mesh_term)


def _d():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _nearest(name):
    """ops.chamfer_nearest on the case: (sums [N,2], idx_x, idx_y) as numpy."""
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    c = chamfer_case(name)
    xl = None if c.xl is None else torch.tensor(c.xl, device=d)
    yl = None if c.yl is None else torch.tensor(c.yl, device=d)
    sums, ix, iy = ops.chamfer_nearest(torch.tensor(c.x, device=d), torch.tensor(c.y, device=d), xl, yl)
    assert ix.dtype == torch.int32 and iy.dtype == torch.int32
    return sums.cpu().numpy(), ix.cpu().numpy(), iy.cpu().numpy()


def _check_indices(name, ix, iy):
    """Equal to the float64 argmin on every row inside the lengths that is no near tie."""
    c, r = chamfer_case(name), chamfer_reference(name)
    for tag, got, want, tie, P, lens in (("idx_x", ix, r["ix"], r["tie_x"], c.P1, c.lx), ("idx_y", iy, r["iy"], r["tie_y"], c.P2, c.ly)):
        live = (np.arange(P)[None] < np.asarray(lens)[:, None]) & ~tie
        bad = int((got != want)[live].sum())
        print("%s %s: %d of %d rows differ from the float64 argmin (%d near ties left out)" % (name, tag, bad, int(live.sum()), int(tie.sum())))
        assert bad == 0, (name, tag)


def _chamfer(name, scale=1.0):
    _check_indices(name, *_nearest(name)[1:])
    check_chamfer(name, run_chamfer(name, _d(), scale), name, scale, host=chamfer_host(name))


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("P1,P2", SIZE_PAIRS)
def test_chamfer_sizes(P1, P2, N):
    _chamfer("n%d-%dx%d" % (N, P1, P2))


@pytest.mark.gpu
@pytest.mark.parametrize("P1,P2", BOUND_PAIRS)
def test_chamfer_tile_and_lds_bounds(P1, P2):
    """Either side of the 1024-candidate round of the forward and of the backward's LDS sizes (module docstring)."""
    assert CH_ROUND == 1024 and 12 * (LDS_64K_P - 1) <= 64 * 1024 < 12 * LDS_64K_P and 12 * CH_BWD_LDS_MAX_P == 150 * 1024
    _chamfer("n1-%dx%d" % (P1, P2))


@pytest.mark.gpu
def test_chamfer_lengths_and_nan_padding():
    """Lengths shorter than P with NaN in the padding (clouds of length 1 and 0 among them): the values are those of the
    truncated clouds, the padded gradient rows are exactly 0 (check_chamfer asserts it), a length of 0 gives a sum of 0."""
    sums, ix, iy = _nearest("lengths")
    c = chamfer_case("lengths")
    assert np.isfinite(sums).all()
    assert not sums[3].any() and not sums[4].any()                      # y_len = 0 / x_len = 0
    assert (ix[3, :20] == -1).all() and (iy[4, :9] == -1).all()
    _check_indices("lengths", ix, iy)
    check_chamfer("lengths", run_chamfer("lengths", _d()), "lengths", host=chamfer_host("lengths"))
    assert c.xl[1] == 1 and c.yl[2] == 1


@pytest.mark.gpu
def test_chamfer_ties_and_duplicates():
    """Exact duplicates: y[3] == y[7] == y[290] (the last one in another wave's quarter of the cloud) == x[5]; x[6] ==
    x[9].  The lowest index wins; the gradients are finite, and 0 where the only term is a pair at distance 0."""
    sums, ix, iy = _nearest("ties")
    r = chamfer_reference("ties")
    assert ix[0, 5] == 3 and iy[0, 3] == 5 and iy[0, 7] == 5 and iy[0, 290] == 5
    chose = np.nonzero((r["iy"][0] == 6) | (r["iy"][0] == 9))[0]
    assert chose.size > 0 and (iy[0, chose] == 6).all()                 # x[6] before its copy x[9]
    assert np.array_equal(ix, r["ix"]) and np.array_equal(iy, r["iy"])
    got = run_chamfer("ties", _d())
    assert np.isfinite(got[1]).all() and np.isfinite(got[2]).all()
    assert not got[2][0, 7].any() and not got[2][0, 290].any()
    check_chamfer("ties", got, "ties", host=chamfer_host("ties"))


@pytest.mark.gpu
def test_chamfer_reproducible_and_scaled_backward():
    """Two forward runs are bit-identical (ticket finish: no float atomics), the ticket words are back at zero, and the
    backward through loss * 3 is three times the gradient."""
    from acfm_video_3d_reconstruction_amd import ops
    name = "n3-257x1000"
    a, b = _nearest(name), _nearest(name)
    assert all(np.array_equal(p, q) for p, q in zip(a, b))
    assert ops.loss_tickets_clean()
    check_chamfer(name + " x3", run_chamfer(name, _d(), 3.0), name, 3.0, host=chamfer_host(name))
    assert ops.loss_tickets_clean()


@pytest.mark.gpu
def test_chamfer_reductions_on_the_gpu():
    """The default reductions (mean / mean) and weights with batch_reduction "mean" agree with the host path."""
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.loss import chamfer_distance
    d = _d()
    c = chamfer_case("lengths")
    keep = [0, 1, 2]
    args = lambda dev: (torch.tensor(c.x[keep], device=dev), torch.tensor(c.y[keep], device=dev),
                        torch.tensor(c.xl[keep], device=dev), torch.tensor(c.yl[keep], device=dev))
    for kw in ({}, {"batch_reduction": "sum", "point_reduction": "sum"}, {"batch_reduction": None}):
        for w in (None, c.w[keep]):
            got = chamfer_distance(*args(d), weights=None if w is None else torch.tensor(w, device=d), **kw)[0]
            want = chamfer_distance(*args("cpu"), weights=None if w is None else torch.tensor(w), **kw)[0]
            print("reductions %s weights=%s: %s vs host %s" % (kw, w is not None, got.cpu().numpy(), want.numpy()))
            np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), rtol=1e-5)


# ======================================================================================== edge length, normal consistency
@pytest.mark.gpu
@pytest.mark.parametrize("name,target", EDGE_RUNS)
def test_edge_loss(name, target):
    """mesh_edge_loss on two equal 3 x 3 / 9 x 7 / 65 x 64 jittered grids (padded tensors), the three in one batch
    (per-mesh weights differ), and a batch with a zero-length edge (finite, subgradient 0), at target_length 0 and 0.1."""
    scale = 3.0 if name == "eq-9x7" else 1.0
    loss, grad = run_mesh_term(name, "edge", _d(), target, scale)
    check_mesh_term("%s edge target %.1f" % (name, target), loss.item(), grad, name, "edge", target, scale)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NORMAL_RUNS)
def test_normal_consistency(name):
    """mesh_normal_consistency on the grids (boundary edges give no pair), the closed ico_sphere(2), the fan of three
    faces on one edge (three pairs), a batch with one exactly degenerate face (everything finite; the vertices of its
    pairs are left out of the gradient bars) and a batch of two different topologies."""
    scale = 3.0 if name == "eq-9x7" else 1.0
    loss, grad = run_mesh_term(name, "normal", _d(), scale=scale)
    check_mesh_term(name + " normal", loss.item(), grad, name, "normal", scale=scale)


@pytest.mark.gpu
def test_mesh_terms_lists_float_faces_and_no_pairs():
    """The same batch as a list of meshes with float faces (as fit_verts_to_mesh builds it) gives the padded batch's bits
    in the forward; a mesh without a shared edge gives the zero tensor; two runs are bit-identical."""
    from acfm_video_3d_reconstruction_amd import ops
    from acfm_video_3d_reconstruction_amd import pytorch3d_shim as p3d
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.structures import Meshes
    d = _d()
    c = mesh_case("eq-9x7")
    as_list = Meshes(verts=[torch.tensor(v, device=d) for v in c.verts], faces=[torch.tensor(f, device=d).float() for f in c.faces])
    padded, _ = c.meshes(d)
    for fn in (p3d.loss.mesh_edge_loss, p3d.loss.mesh_normal_consistency):
        a, b = fn(as_list), fn(padded)
        assert torch.equal(a, b) and torch.equal(fn(as_list), a), fn.__name__
    ms, _ = mesh_case("no-shared-edge").meshes(d)
    z = p3d.loss.mesh_normal_consistency(ms)
    assert z.shape == (1,) and z.item() == 0.0 and z.requires_grad and z.is_cuda
    assert ops.loss_tickets_clean()


# ===================================================================================================== end to end
@pytest.mark.gpu
def test_fit_sphere_to_ellipsoid():
    """ico_sphere(3) plus a learnable offset fitted to an ellipsoid: 30 SGD steps of chamfer + edge + 0.01 normal + 0.1
    Laplacian with 1000 samples a side; every term finite at every step, the chamfer term falls."""
    from acfm_video_3d_reconstruction_amd import pytorch3d_shim as p3d
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.structures import Meshes
    d = _d()
    torch.manual_seed(5)
    sphere = p3d.utils.ico_sphere(3, d)
    base, faces = sphere.verts_list()[0], sphere.faces_list()[0]
    target = Meshes(verts=[base * torch.tensor([1.0, 0.6, 0.4], device=d)], faces=[faces])
    offset = torch.zeros_like(base, requires_grad=True)
    opt = torch.optim.SGD([offset], lr=1.0, momentum=0.9)
    history = []
    for step in range(30):
        opt.zero_grad()
        mesh = Meshes(verts=[base + offset], faces=[faces])
        chamfer = p3d.loss.chamfer_distance(p3d.ops.sample_points_from_meshes(target, 1000),
                                            p3d.ops.sample_points_from_meshes(mesh, 1000))[0]
        terms = [chamfer, p3d.loss.mesh_edge_loss(mesh), p3d.loss.mesh_normal_consistency(mesh),
                 p3d.loss.mesh_laplacian_smoothing(mesh, "uniform")]
        (terms[0] + terms[1] + 0.01 * terms[2] + 0.1 * terms[3]).backward()
        opt.step()
        history.append(torch.stack([t.detach().reshape(()) for t in terms]))
    history = torch.stack(history).cpu().numpy()
    print("chamfer, edge, normal, laplacian at steps 0 / 29: %s / %s" % (history[0], history[-1]))
    assert np.isfinite(history).all() and bool(torch.isfinite(offset).all())
    assert history[-1, 0] < history[0, 0]
