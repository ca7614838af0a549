"""GPU: the mesh priors (csrc/acfm_mesh.hip), the template-fit terms (csrc/acfm_fit.hip), surface sampling and the
boundary draw on hostile, fenced memory: tests/guards.py run_case.

The template-fit forwards end in a ticket finish (a fixed-order sum), so their values, indices and samples are bits.
The Laplacian and rigidity forwards add their loss with float atomics, and the backwards of all these terms scatter
with float atomics; none has a deterministic mode.  Those results are held, in every run, to the float64 references
and bars of tests/test_gpu_mesh_priors.py and tests/test_shim_template_fit.py -- and still to completeness and the
fences."""
import numpy as np
import pytest
import torch

import guards
from test_gpu_mesh_priors import (_guarded, _laplacian_input, check_lap, check_rigid, lap_case, rigid_case,
                                  rigid_reference)
from test_shim_template_fit import (CH_BWD_LDS_MAX_P, REL_L2_FLOOR, VALUE_RTOL, ChamferCase, _nearest64, chamfer_case,
                                    chamfer_host, check_chamfer, check_grad, check_mesh_term, edges_of, mesh_case, pairs_of)

pytestmark = pytest.mark.gpu
_report = guards.module_report(__name__)


def _d():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, d, grad=False):
    return torch.tensor(a, device=d, requires_grad=grad)


# ------------------------------------------------------------------------------------------------ mesh priors
@pytest.mark.parametrize("V", [5, 65])
def test_cot_laplacian(V):
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    v, f, _valid = _laplacian_input(V)       # (out-of-range and repeated ids among the faces)

    def fn(inp):
        return dict(L=ops.cot_laplacian(inp(_t(np.asarray(v, np.float32), d)), torch.as_tensor(np.asarray(f)).to(d)))
    guards.run_case(fn)


@pytest.mark.parametrize("method", ["cot", "uniform"])
@pytest.mark.parametrize("name,hinted", [("eq-9x7", True), ("eq-9x7", False), ("unequal", False)])
def test_laplacian_smoothing(name, hinted, method):
    """laplacian_smoothing_sum on two 9 x 7 grids (63 vertices: the tails of every loop) with the per-mesh LDS kernels
    and, without the layout hint, on the global path; and on three meshes of different sizes."""
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    c = lap_case(name)
    conn = torch.from_numpy(np.ascontiguousarray(c.conn(method))).to(d)
    vpm, fpm = (c.sizes[0], c.faces[0].shape[0]) if hinted else (0, 0)

    def fn(inp):
        v = inp(_t(c.vp, d, True))
        loss = ops.laplacian_smoothing_sum(v, conn, inp(_t(c.vw.astype(np.float32), d)), 0 if method == "cot" else 1,
                                           vpm, fpm) / c.N
        gv, = torch.autograd.grad(loss, v)
        check_lap("%s %s hinted=%s" % (name, method, hinted), loss.item(), gv.cpu().numpy(), name, method)
        return dict(loss=loss, gv=gv)
    plain, held = guards.run_case(fn, loose=("loss", "gv"))
    if hinted and method == "cot":           # the ALLOWED entry: Wv of the per-mesh path stays unwritten
        for g in held.values():
            assert guards.still_poisoned(g, "mesh_terms.py:_LaplacianSmoothing.forward:state") == 3 * c.P


@pytest.mark.parametrize("name,hinted,template_grad", [("runs", True, True), ("runs", False, True), ("one-edge", True, False)])
def test_edge_rigidity(name, hinted, template_grad):
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    c = rigid_case(name)

    def fn(inp):
        v, vt = inp(_t(c.v, d, True)), inp(_t(c.vt, d, template_grad))
        loss = ops.edge_rigidity_sum(v, _guarded(c.e, d), vt, _guarded(c.et, d), c.vpm if hinted else 0)
        gs = torch.autograd.grad(loss, (v, vt) if template_grad else (v,))
        check_rigid("%s hinted=%s" % (name, hinted),
                    (loss.item(), gs[0].cpu().numpy(), gs[1].cpu().numpy() if template_grad else None), rigid_reference(name))
        return dict(loss=loss, gv=gs[0], gvt=gs[1] if template_grad else None)
    guards.run_case(fn, loose=("loss", "gv", "gvt"))


def _term_inputs(name, term):
    """Packed vertices, the connectivity and the per-entry weights 1 / (entries of its mesh), as the shim forms them."""
    c = mesh_case(name)
    conn = edges_of(c.fp) if term == "edge" else pairs_of(c.fp)
    mesh = c.mesh_of_vert[conn[:, 0]]
    w = (1.0 / np.bincount(mesh, minlength=c.N)[mesh]).astype(np.float32)
    return c, conn, w


@pytest.mark.parametrize("term,target", [("edge", 0.0), ("edge", 0.1), ("normal", 0.0)])
@pytest.mark.parametrize("name", ["eq-3x3", "eq-9x7", "unequal"])
def test_edge_length_and_normal_consistency(name, term, target):
    """edge_length_sum / normal_consistency_sum; the connectivity lies in a tensor with one spare row (a repeat of the
    last one) behind it, so a kernel that goes one entry too far adds a real entry and misses its reference."""
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    c, conn, w = _term_inputs(name, term)
    tc = _guarded(conn, d)

    def fn(inp):
        v = inp(_t(c.vp, d, True))
        tw = inp(_t(w, d))
        loss = (ops.edge_length_sum(v, tc, tw, target) if term == "edge" else ops.normal_consistency_sum(v, tc, tw)) / c.N
        gv, = torch.autograd.grad(loss, v)
        check_mesh_term("%s %s %.1f" % (name, term, target), loss.item(), gv.cpu().numpy(), name, term, target)
        return dict(loss=loss, gv=gv)
    guards.run_case(fn, loose=("gv",))


# ------------------------------------------------------------------------------------------------ chamfer
CHAMFER = ["n1-63x65", "n3-63x65", "n1-1025x64", "lengths", "n1-12801x64"]


@pytest.mark.parametrize("name", CHAMFER)
def test_chamfer(name):
    """chamfer_nearest / chamfer_sums either side of a 64-point workgroup, past one 1024-candidate round, with lengths
    (NaN in the padding) and at 12801 points, where the backward is the global-atomic pair k_chamfer_bwd_own /
    k_chamfer_bwd_scatter.  sums and both index planes inside the lengths are bits; the gradients against float64."""
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    c = chamfer_case(name)
    xl = None if c.xl is None else torch.tensor(c.xl, device=d)
    yl = None if c.yl is None else torch.tensor(c.yl, device=d)
    live_x = torch.from_numpy(np.arange(c.P1)[None] < np.asarray(c.lx)[:, None]).to(d)
    live_y = torch.from_numpy(np.arange(c.P2)[None] < np.asarray(c.ly)[:, None]).to(d)
    host = chamfer_host(name) if c.P1 * c.P2 <= 70000 else None

    def fn(inp):
        x, y = inp(_t(c.x, d, True)), inp(_t(c.y, d, True))
        sums, ix, iy = ops.chamfer_nearest(x, y, xl, yl)
        loss = (sums.sum(1) * _t(c.w, d))
        gx, gy = torch.autograd.grad(loss.sum(), (x, y))
        check_chamfer(name, (loss.detach().cpu().numpy(), gx.cpu().numpy(), gy.cpu().numpy()), name, host=host)
        # rows at or past a length hold no value (ops.chamfer_nearest): compared inside the lengths
        return dict(sums=sums, ix=torch.where(live_x, ix, -7), iy=torch.where(live_y, iy, -7), gx=gx, gy=gy)
    plain, held = guards.run_case(fn, loose=("gx", "gy"))
    if name == "lengths":                    # the ALLOWED entries: the rows past the lengths are there and unwritten
        for g in held.values():
            assert guards.still_poisoned(g, "mesh_terms.py:_Chamfer.forward:ix") == int((~live_x).sum())
            assert guards.still_poisoned(g, "mesh_terms.py:_Chamfer.forward:iy") == int((~live_y).sum())


def _chamfer_reference(c):
    """chamfer_reference of tests/test_shim_template_fit.py (float64 brute force) for a case that has no name there."""
    loss = np.zeros(c.N)
    gx, gy = np.zeros((c.N, c.P1, 3)), np.zeros((c.N, c.P2, 3))
    sx, sy = np.zeros((c.N, c.P1), bool), np.zeros((c.N, c.P2), bool)
    for n in range(c.N):
        lx, ly = int(c.lx[n]), int(c.ly[n])
        x, y = c.x[n, :lx].astype(np.float64), c.y[n, :ly].astype(np.float64)
        for q, t, gq, gt, sq, st in ((x, y, gx[n], gy[n], sx[n], sy[n]), (y, x, gy[n], gx[n], sy[n], sx[n])):
            idx, best, tie, second = _nearest64(q, t)
            loss[n] += c.w[n] * best.sum()
            g = 2.0 * c.w[n] * (q - t[idx])
            gq[:q.shape[0]] += g
            np.add.at(gt, idx, -g)
            sq[:q.shape[0]] |= tie
            st[idx[tie]] = True
            st[second[tie]] = True
    return loss, gx, gy, sx, sy


def test_chamfer_global_backward_with_lengths():
    """12801 points with lengths below P on both sides (NaN in the padding): k_chamfer_bwd_own writes the padded rows'
    zeros itself, k_chamfer_bwd_scatter adds behind it.  The float64 brute force and the bars (value 1e-5; gradients
    rtol 1e-3, 1e-5 of the largest entry, relative L2 at the floor) are those of test_shim_template_fit.py."""
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    P1, P2 = CH_BWD_LDS_MAX_P + 1, 64
    rng = np.random.default_rng(12801)
    x = rng.uniform(-1, 1, (2, P1, 3)).astype(np.float32)
    y = rng.uniform(-1, 1, (2, P2, 3)).astype(np.float32)
    xl, yl = np.array([P1, 9000]), np.array([40, P2])
    for n in range(2):
        x[n, xl[n]:] = np.nan
        y[n, yl[n]:] = np.nan
    c = ChamferCase(x, y, xl, yl, rng.uniform(0.5, 2.0, 2).astype(np.float32))
    loss64, gx64, gy64, sx, sy = _chamfer_reference(c)
    txl, tyl = torch.tensor(xl, device=d), torch.tensor(yl, device=d)
    pad_x, pad_y = np.arange(P1)[None] >= xl[:, None], np.arange(P2)[None] >= yl[:, None]

    def fn(inp):
        tx, ty = inp(_t(c.x, d, True)), inp(_t(c.y, d, True))
        sums = ops.chamfer_sums(tx, ty, txl, tyl)
        loss = sums.sum(1) * _t(c.w, d)
        gx, gy = torch.autograd.grad(loss.sum(), (tx, ty))
        np.testing.assert_allclose(loss.detach().cpu().numpy(), loss64, rtol=VALUE_RTOL, atol=0)
        for tag, g, r, skip, pad in (("grad_x", gx, gx64, sx, pad_x), ("grad_y", gy, gy64, sy, pad_y)):
            g = g.cpu().numpy()
            assert not g[pad].any(), "%s: padded rows must be exactly 0" % tag
            check_grad("12801 with lengths " + tag, g, r, ~skip, REL_L2_FLOOR)
        return dict(sums=sums, gx=gx, gy=gy)
    guards.run_case(fn, loose=("gx", "gy"))


# ------------------------------------------------------------------------------------------------ sampling, the draw
def test_sample_points_from_meshes():
    from acfm_video_3d_reconstruction_amd import pytorch3d_shim as p3d
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.structures import Meshes
    d = _d()
    c = mesh_case("eq-9x7")
    faces = torch.from_numpy(np.stack(c.faces)).to(d)

    def fn(inp):
        v = inp(_t(np.stack(c.verts), d, True))
        torch.manual_seed(11)
        pts, nrm = p3d.ops.sample_points_from_meshes(Meshes(verts=v, faces=faces), 65, return_normals=True)
        gv, = torch.autograd.grad((pts * pts).sum() + nrm.sum(), v)
        return dict(pts=pts, nrm=nrm, gv=gv)
    guards.run_case(fn, loose=("gv",))


@pytest.mark.parametrize("counts,per_mesh", [(None, False), ((40, 7, 65), True), ((40, 7, 65), False), ((100, 100, 100), True)])
def test_boundary_subset(counts, per_mesh):
    """boundary_subset with P_r < n (a -1 tail), = n and > n, against boundary_sampling.subset_host index for index
    in the plain run, and bit for bit between the runs."""
    from acfm_video_3d_reconstruction_amd import ops
    d = _d()
    P, S = 65, 40
    tc = None if counts is None else torch.tensor(counts, dtype=torch.int32, device=d)

    def fn(inp):
        state = torch.tensor([5, 2], dtype=torch.int64, device=d)
        sel = ops.boundary_subset(state, P, S, counts=tc, per_mesh=per_mesh)
        return dict(sel=sel, state=state)
    plain, _ = guards.run_case(fn)
    sel = plain["sel"].cpu().numpy()
    assert plain["state"].tolist() == [5, 3]
    rows = [min(P, n) for n in counts] if per_mesh else [min(P, max(counts)) if counts else P]
    for r, pr in enumerate(rows):
        k = min(S, pr)
        assert (np.diff(sel[r, :k]) > 0).all() and sel[r, 0] >= 0 and sel[r, k - 1] < pr and (sel[r, k:] == -1).all()
