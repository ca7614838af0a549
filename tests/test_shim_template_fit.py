"""The template fit's slice of the shim on host tensors (no GPU): pytorch3d.utils.ico_sphere, io.save_obj,
ops.sample_points_from_meshes, loss.chamfer_distance / mesh_edge_loss / mesh_normal_consistency and the new Meshes
queries, against float64 restatements written here.  The inputs and helpers of tests/test_gpu_template_fit.py live in
this file: every GPU input is first put through the float32 host path at the GPU tests' bars.

Bars (the suite's): values rtol 1e-5 against float64; gradients rtol 1e-3 with atol = 1e-5 of the largest reference
entry; gradient relative L2 <= max(1e-5, 4 x the host path's).  The value of the normal term is 1 - cos of nearly
parallel normals, which cancels in float32: its bar is max(1e-5, 4 x the host path's own relative error on the input).
Chamfer rows whose best and second-best squared distances differ by less than 1e-5 relative in float64 are left out of
the index and gradient comparisons (with the candidates they hesitate between); they may not exceed 0.5 % of the rows of
a case, which test_chamfer_inputs_have_few_near_ties asserts for every input."""
import functools
import io
import sys

import numpy as np
import pytest
import torch

from test_gpu_mesh_priors import grid

VALUE_RTOL = 1e-5
GRAD_RTOL = 1e-3
GRAD_FRAC = 1e-5
REL_L2_FLOOR = 1e-5
REL_L2_FACTOR = 4.0
TIE_GAP = 1e-5
TIE_SHARE = 0.005
# the sizes at which the chamfer kernels take another path (csrc/acfm_fit.hip)
CH_Q = 64                    # query points per workgroup (k_chamfer)
CH_ROUND = 4 * 256           # candidates per round: four waves x a tile of CH_TILE = 256 (a wave's quarter of the cloud
                             # needs a second round past 256, i.e. the cloud past 1024)
CH_BWD_LDS_MAX_P = 12800     # 12 B of LDS per point <= 150 KB (k_chamfer_bwd); past it k_chamfer_bwd_own / _scatter
LDS_64K_P = 5462             # the first size whose 12 B per point pass 64 KB of dynamic LDS


# =============================================================================================== chamfer: inputs
class ChamferCase:
    def __init__(self, x, y, xl=None, yl=None, w=None):
        self.x, self.y, self.xl, self.yl = x, y, xl, yl
        self.N, self.P1, self.P2 = x.shape[0], x.shape[1], y.shape[1]
        self.w = np.ones(self.N, np.float32) if w is None else w
        self.lx = np.full(self.N, self.P1) if xl is None else np.clip(xl, 0, self.P1)
        self.ly = np.full(self.N, self.P2) if yl is None else np.clip(yl, 0, self.P2)


SIZE_PAIRS = [(1, 1), (1, 64), (63, 65), (64, 64), (257, 1000), (1000, 2049)]
BOUND_PAIRS = [(64, CH_ROUND), (64, CH_ROUND + 1), (CH_ROUND + 1, 64), (LDS_64K_P, 64), (CH_BWD_LDS_MAX_P, 64),
               (CH_BWD_LDS_MAX_P + 1, 64), (64, CH_BWD_LDS_MAX_P + 1)]
CHAMFER_NAMES = (["n%d-%dx%d" % (n, a, b) for n in (1, 3) for a, b in SIZE_PAIRS] +
                 ["n1-%dx%d" % ab for ab in BOUND_PAIRS] + ["lengths", "ties"])


@functools.lru_cache(maxsize=None)
def chamfer_case(name):
    if name == "lengths":            # NaN padding; clouds of length 1 on either side, and of length 0 (its sums are 0)
        rng = np.random.default_rng(21)
        x = rng.uniform(-1, 1, (5, 70, 3)).astype(np.float32)
        y = rng.uniform(-1, 1, (5, 130, 3)).astype(np.float32)
        xl, yl = np.array([70, 1, 33, 20, 0]), np.array([5, 130, 1, 0, 9])
        for n in range(5):
            x[n, xl[n]:] = np.nan
            y[n, yl[n]:] = np.nan
        return ChamferCase(x, y, xl, yl, rng.uniform(0.5, 2.0, 5).astype(np.float32))
    if name == "ties":               # exact duplicates: y[0,3] == y[0,7]; x[0,5] == y[0,3]; x[0,6] == x[0,9]
        rng = np.random.default_rng(22)
        x = rng.uniform(-1, 1, (1, 40, 3)).astype(np.float32)
        y = rng.uniform(-1, 1, (1, 300, 3)).astype(np.float32)
        y[0, 7] = y[0, 3]
        y[0, 290] = y[0, 3]          # the third copy lies in another wave's quarter of the cloud
        x[0, 5] = y[0, 3]
        x[0, 9] = x[0, 6]
        return ChamferCase(x, y)
    n, rest = name.split("-")
    N, (P1, P2) = int(n[1:]), (int(v) for v in rest.split("x"))
    rng = np.random.default_rng(1000 * N + 7 * P1 + P2)
    w = rng.uniform(0.5, 2.0, N).astype(np.float32)
    return ChamferCase(rng.uniform(-1, 1, (N, P1, 3)).astype(np.float32), rng.uniform(-1, 1, (N, P2, 3)).astype(np.float32), w=w)


def _nearest64(q, c):
    """q [A,3], c [B,3] float64, B >= 1 -> (index of the first minimum, its value, near-tie flag, the runner-up).  A
    runner-up that is a bit-exact copy of the winner is no near tie: every arithmetic gives the two the same distance,
    and the lowest index must win."""
    d = ((q[:, None, :] - c[None, :, :]) ** 2).sum(-1)
    idx = np.argmin(d, 1)                                    # the first occurrence
    best = d[np.arange(d.shape[0]), idx]
    if d.shape[1] == 1:
        return idx, best, np.zeros(d.shape[0], bool), idx
    masked = d.copy()
    masked[np.arange(d.shape[0]), idx] = np.inf
    second_i = np.argmin(masked, 1)
    second = masked[np.arange(d.shape[0]), second_i]
    return idx, best, ((second - best) <= TIE_GAP * second) & ~(c[idx] == c[second_i]).all(1), second_i


@functools.lru_cache(maxsize=None)
def chamfer_reference(name):
    """float64 brute force, computed once: per-cloud loss w (cham_x + cham_y) [N], the indices (-1 where there is no
    candidate), the gradients of sum_n loss[n], and per cloud the rows to leave out of the index / gradient comparison
    (near ties and the two candidates each hesitates between)."""
    c = chamfer_case(name)
    loss = np.zeros(c.N)
    ix, iy = np.full((c.N, c.P1), -1), np.full((c.N, c.P2), -1)
    gx, gy = np.zeros((c.N, c.P1, 3)), np.zeros((c.N, c.P2, 3))
    tx, ty = np.zeros((c.N, c.P1), bool), np.zeros((c.N, c.P2), bool)     # near-tie rows
    sx, sy = np.zeros((c.N, c.P1), bool), np.zeros((c.N, c.P2), bool)     # rows left out of the gradient comparison
    for n in range(c.N):
        lx, ly = int(c.lx[n]), int(c.ly[n])
        if lx == 0 or ly == 0:
            continue
        x, y = c.x[n, :lx].astype(np.float64), c.y[n, :ly].astype(np.float64)
        for (q, t, iq, gq, gt, tq, sq, st) in ((x, y, ix[n], gx[n], gy[n], tx[n], sx[n], sy[n]),
                                               (y, x, iy[n], gy[n], gx[n], ty[n], sy[n], sx[n])):
            idx, best, tie, second = _nearest64(q, t)
            iq[:q.shape[0]] = idx
            loss[n] += c.w[n] * best.sum()
            g = 2.0 * c.w[n] * (q - t[idx])
            gq[:q.shape[0]] += g
            np.add.at(gt, idx, -g)
            tq[:q.shape[0]] = tie
            sq[:q.shape[0]] |= tie
            st[idx[tie]] = True
            st[second[tie]] = True
    return dict(loss=loss, ix=ix, iy=iy, gx=gx, gy=gy, tie_x=tx, tie_y=ty, skip_x=sx, skip_y=sy)


def run_chamfer(name, device, scale=1.0):
    """The public operator on `device`: per-cloud loss [N] (batch_reduction None, point_reduction "sum", weights) and
    the gradients of (sum_n loss[n]) * scale."""
    from acfm_video_3d_reconstruction_amd import pytorch3d_shim as p3d
    c = chamfer_case(name)
    x = torch.tensor(c.x, device=device, requires_grad=True)
    y = torch.tensor(c.y, device=device, requires_grad=True)
    xl = None if c.xl is None else torch.tensor(c.xl, device=device)
    yl = None if c.yl is None else torch.tensor(c.yl, device=device)
    loss, none = p3d.loss.chamfer_distance(x, y, xl, yl, weights=torch.tensor(c.w, device=device), batch_reduction=None,
                                           point_reduction="sum")
    assert none is None and loss.shape == (c.N,)
    (loss.sum() * scale).backward()
    return loss.detach().cpu().numpy(), x.grad.cpu().numpy(), y.grad.cpu().numpy()


@functools.lru_cache(maxsize=None)
def chamfer_host(name):
    return run_chamfer(name, torch.device("cpu"))


def _rel_l2(got, ref, keep):
    got, ref = np.asarray(got, np.float64)[keep], np.asarray(ref, np.float64)[keep]
    nrm = float(np.linalg.norm(ref))
    return float(np.linalg.norm(got - ref)) / nrm if nrm > 0 else float(np.linalg.norm(got - ref))


def check_grad(what, got, ref, keep, l2_bar):
    """rtol / atol on the kept rows (atol from the largest kept reference entry) and the relative L2 bar."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.isfinite(got).all(), what
    if not keep.any():
        return
    gmax = float(np.abs(ref[keep]).max())
    rel = _rel_l2(got, ref, keep)
    print("%s: max err %.2e of max (atol %.0e of max, rtol %.0e)  rel L2 %.2e (bar %.2e)"
          % (what, float(np.abs(got - ref)[keep].max()) / max(gmax, 1e-300), GRAD_FRAC, GRAD_RTOL, rel, l2_bar))
    np.testing.assert_allclose(got[keep], ref[keep], rtol=GRAD_RTOL, atol=GRAD_FRAC * gmax, err_msg=what)
    assert rel <= l2_bar, (what, rel, l2_bar)


def check_chamfer(what, got, name, scale=1.0, host=None):
    """got = (loss [N], grad_x, grad_y) against the float64 reference; host: the host path's result for the L2 bar
    (None: the floor alone, which is what the host path itself is held to)."""
    c, ref = chamfer_case(name), chamfer_reference(name)
    loss, gx, gy = got
    err = np.abs(loss - ref["loss"]) / np.maximum(np.abs(ref["loss"]), 1e-300)
    print("%s: value rel err %.2e (bar %.0e)" % (what, float(err.max()), VALUE_RTOL))
    assert np.isfinite(loss).all(), what
    np.testing.assert_allclose(loss, ref["loss"], rtol=VALUE_RTOL, atol=0, err_msg=what)
    for tag, g, r, skip, P, lens in (("grad_x", gx, ref["gx"], ref["skip_x"], c.P1, c.lx),
                                     ("grad_y", gy, ref["gy"], ref["skip_y"], c.P2, c.ly)):
        pad = np.arange(P)[None] >= np.asarray(lens)[:, None]
        assert not np.asarray(g)[pad].any(), "%s %s: padded rows must be exactly 0" % (what, tag)
        bar = REL_L2_FLOOR
        if host is not None:
            bar = max(REL_L2_FLOOR, REL_L2_FACTOR * _rel_l2(host[1 if tag == "grad_x" else 2], r, ~skip))
        check_grad("%s %s" % (what, tag), g, r * scale, ~skip, bar)


# ================================================================================== edge / normal terms: inputs
class MeshCase:
    """A batch of meshes (float32 verts, local int64 faces)."""

    def __init__(self, verts, faces):
        self.verts, self.faces = verts, faces
        self.sizes = [v.shape[0] for v in verts]
        self.N, self.P = len(verts), sum(self.sizes)
        first = np.cumsum([0] + self.sizes[:-1])
        self.vp = np.concatenate(verts, 0)
        self.fp = np.concatenate([f + o for f, o in zip(faces, first)], 0)
        self.mesh_of_vert = np.repeat(np.arange(self.N), self.sizes)
        self.equal = len(set(self.sizes)) == 1 and len({f.shape[0] for f in faces}) == 1

    def meshes(self, device, padded=None):
        """-> (Meshes, the leaf tensors); equal-sized batches as padded tensors (as the trainer builds them)."""
        from acfm_video_3d_reconstruction_amd.pytorch3d_shim.structures import Meshes
        if self.equal if padded is None else padded:
            vs = [torch.tensor(np.stack(self.verts), device=device, requires_grad=True)]
            return Meshes(verts=vs[0], faces=torch.from_numpy(np.stack(self.faces)).to(device)), vs
        vs = [torch.tensor(v, device=device, requires_grad=True) for v in self.verts]
        return Meshes(verts=vs, faces=[torch.from_numpy(f).to(device) for f in self.faces]), vs


def _perturbed(v, n, seed):
    rng = np.random.default_rng(seed)
    return [v] + [(v + rng.uniform(-1e-3, 1e-3, v.shape)).astype(np.float32) for _ in range(n - 1)]


def _ico(level):
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.utils import ico_sphere
    m = ico_sphere(level)
    return m.verts_list()[0].numpy().copy(), m.faces_list()[0].numpy().copy()


GRIDS = [(3, 3), (9, 7), (65, 64)]
MESH_NAMES = ["eq-%dx%d" % ab for ab in GRIDS] + ["unequal", "zero-edge", "ico2", "fan", "no-shared-edge", "two-topologies"]


@functools.lru_cache(maxsize=None)
def mesh_case(name):
    if name.startswith("eq-"):                      # two equal-sized jittered grids
        a, b = (int(x) for x in name[3:].split("x"))
        v, f = grid(a, b)
        return MeshCase(_perturbed(v, 2, a + b), [f, f])
    if name == "unequal":                           # the three grids in one batch: per-mesh weights differ
        vf = [grid(a, b) for a, b in GRIDS]
        return MeshCase([v for v, _ in vf], [f for _, f in vf])
    if name == "zero-edge":                         # vertex 1 of mesh 0 = a bit-exact copy of vertex 0: the edge (0, 1) has
        v, f = grid(9, 7)                           # length 0 and the face that holds both has a zero normal
        vs = _perturbed(v, 2, 16)
        vs[0] = vs[0].copy()
        vs[0][1] = vs[0][0]
        assert int(((f == 0).any(1) & (f == 1).any(1)).sum()) == 1
        return MeshCase(vs, [f, f])
    if name == "ico2":                              # closed: every edge gives one pair
        v, f = _ico(2)
        rng = np.random.default_rng(3)
        return MeshCase([(v + rng.uniform(-0.02, 0.02, v.shape)).astype(np.float32)], [f])
    if name == "fan":                               # three faces on the edge (0, 1): three pairs
        v = np.array([[0, 0, 0], [1, 0, 0.1], [0.4, 1, 0], [0.5, -0.2, 0.9], [0.6, -0.8, -0.5]], np.float32)
        return MeshCase([v], [np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], np.int64)])
    if name == "no-shared-edge":                    # two triangles that meet in one vertex: no pair
        v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [-1, 0, 0.5], [0, -1, 0.2]], np.float32)
        return MeshCase([v], [np.array([[0, 1, 2], [0, 3, 4]], np.int64)])
    if name == "two-topologies":                    # a closed sphere and an open grid in one batch
        v0, f0 = _ico(1)
        v1, f1 = grid(9, 7)
        return MeshCase([v0, v1], [f0, f1])
    raise KeyError(name)


def edges_of(fp):
    """Unique (min, max) vertex pairs of packed faces, lexicographic."""
    e = np.concatenate([fp[:, [1, 2]], fp[:, [2, 0]], fp[:, [0, 1]]], 0)
    return np.unique(np.sort(e, 1), axis=0)


def pairs_of(fp):
    """[Q,4] (a, b, c, d): for every edge a < b in m >= 2 faces every unordered pair of the faces' third vertices; plain
    loops over a dictionary, independent of Meshes.normal_pairs_packed."""
    third = {}
    for f in fp.tolist():
        for k in range(3):
            a, b, c = f[(k + 1) % 3], f[(k + 2) % 3], f[k]
            if a != b:
                third.setdefault((min(a, b), max(a, b)), []).append(c)
    out = []
    for (a, b), cs in sorted(third.items()):
        out += [(a, b, cs[i], cs[j]) for i in range(len(cs)) for j in range(i + 1, len(cs))]
    return np.array(out, np.int64).reshape(-1, 4)


def ref_edge_loss(verts, edges, w, target):
    d = (verts[edges[:, 0]] - verts[edges[:, 1]]).norm(dim=1)      # torch's norm: subgradient 0 at a zero-length edge
    return (w * (d - target) ** 2).sum()


def ref_normal_loss(verts, quads, w):
    a = verts[quads[:, 0]]
    eb, ec, ed = verts[quads[:, 1]] - a, verts[quads[:, 2]] - a, verts[quads[:, 3]] - a
    n0, n1 = torch.cross(ec, eb, dim=1), -torch.cross(ed, eb, dim=1)
    cos = (n0 * n1).sum(1) / (n0.norm(dim=1) * n1.norm(dim=1)).clamp(min=1e-8)
    return (w * (1.0 - cos)).sum()


@functools.lru_cache(maxsize=None)
def mesh_reference(name, term, target=0.0):
    """(value, gradient [P,3], rows kept in the gradient comparison) of the shim's loss in float64, computed once."""
    c = mesh_case(name)
    v = torch.tensor(c.vp, dtype=torch.float64, requires_grad=True)
    keep = np.ones(c.P, bool)
    if term == "edge":
        conn = edges_of(c.fp)
        mesh = c.mesh_of_vert[conn[:, 0]]
        w = torch.from_numpy(1.0 / np.bincount(mesh, minlength=c.N)[mesh])
        loss = ref_edge_loss(v, torch.from_numpy(conn), w, target) / c.N
    else:
        conn = pairs_of(c.fp)
        if conn.shape[0] == 0:
            return 0.0, np.zeros((c.P, 3)), keep
        mesh = c.mesh_of_vert[conn[:, 0]]
        w = torch.from_numpy(1.0 / np.bincount(mesh, minlength=c.N)[mesh])
        loss = ref_normal_loss(v, torch.from_numpy(conn), w) / c.N
        # a pair with an exactly zero normal: its four vertices are left out of the gradient bar
        p = c.vp.astype(np.float64)
        a = p[conn[:, 0]]
        n0 = np.cross(p[conn[:, 2]] - a, p[conn[:, 1]] - a)
        n1 = np.cross(p[conn[:, 1]] - a, p[conn[:, 3]] - a)
        dead = ~n0.any(1) | ~n1.any(1)
        keep[np.unique(conn[dead])] = False
    loss.backward()
    return loss.item(), v.grad.numpy(), keep


def run_mesh_term(name, term, device, target=0.0, scale=1.0, padded=None):
    from acfm_video_3d_reconstruction_amd import pytorch3d_shim as p3d
    c = mesh_case(name)
    ms, leaves = c.meshes(device, padded)
    loss = p3d.loss.mesh_edge_loss(ms, target) if term == "edge" else p3d.loss.mesh_normal_consistency(ms)
    if not loss.requires_grad or loss.grad_fn is None:             # the zero tensor of a batch without pairs
        return loss, np.zeros((c.P, 3), np.float32)
    (loss * scale).backward()
    return loss, torch.cat([t.grad.reshape(-1, 3) for t in leaves], 0).cpu().numpy()


@functools.lru_cache(maxsize=None)
def mesh_host(name, term, target=0.0):
    loss, grad = run_mesh_term(name, term, torch.device("cpu"), target)
    return float(loss.detach()), grad


def check_mesh_term(what, value, grad, name, term, target=0.0, scale=1.0, host=True):
    """host=True: the bars that depend on the host path's own error are formed; False: the floors alone."""
    ref_v, ref_g, keep = mesh_reference(name, term, target)
    assert np.isfinite(value) and np.isfinite(grad).all(), what
    vbar, l2bar = VALUE_RTOL, REL_L2_FLOOR
    if host:
        hv, hg = mesh_host(name, term, target)
        if term == "normal":
            vbar = max(VALUE_RTOL, 4.0 * abs(hv - ref_v) / max(abs(ref_v), 1e-300))
        l2bar = max(REL_L2_FLOOR, REL_L2_FACTOR * _rel_l2(hg, ref_g, keep))
    print("%s: value rel err %.2e (bar %.2e)" % (what, abs(value - ref_v) / max(abs(ref_v), 1e-300), vbar))
    np.testing.assert_allclose(value, ref_v, rtol=vbar, atol=0, err_msg=what)
    check_grad(what + " grad", grad, ref_g * scale, keep, l2bar)


EDGE_RUNS = [(n, t) for n in ("eq-3x3", "eq-9x7", "eq-65x64", "unequal", "zero-edge") for t in (0.0, 0.1)]
NORMAL_RUNS = ["eq-3x3", "eq-9x7", "eq-65x64", "unequal", "zero-edge", "ico2", "fan", "two-topologies"]


# ======================================================================================================= the tests
def test_six_names_import_after_install():
    from acfm_video_3d_reconstruction_amd import pytorch3d_shim
    saved = {k: sys.modules[k] for k in list(sys.modules) if k == "pytorch3d" or k.startswith("pytorch3d.")}
    try:
        pytorch3d_shim.install(force=True)
        from pytorch3d.io import save_obj
        from pytorch3d.loss import chamfer_distance, mesh_edge_loss, mesh_normal_consistency
        from pytorch3d.ops import sample_points_from_meshes
        from pytorch3d.utils import ico_sphere
        assert save_obj is pytorch3d_shim.io.save_obj and ico_sphere is pytorch3d_shim.utils.ico_sphere
        assert sample_points_from_meshes is pytorch3d_shim.ops.sample_points_from_meshes
        assert chamfer_distance is pytorch3d_shim.loss.chamfer_distance
        assert mesh_edge_loss is pytorch3d_shim.loss.mesh_edge_loss
        assert mesh_normal_consistency is pytorch3d_shim.loss.mesh_normal_consistency
    finally:
        for k in [k for k in sys.modules if k == "pytorch3d" or k.startswith("pytorch3d.")]:
            del sys.modules[k]
        sys.modules.update(saved)


@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_ico_sphere(level):
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.utils import ico_sphere
    m = ico_sphere(level)
    v, f = m.verts_list()[0], m.faces_list()[0]
    assert v.shape == (10 * 4 ** level + 2, 3) and f.shape == (20 * 4 ** level, 3)
    assert v.dtype == torch.float32 and f.dtype == torch.int64
    assert float((v.double().norm(dim=1) - 1).abs().max()) <= 1e-6
    e = np.sort(np.concatenate([f.numpy()[:, [1, 2]], f.numpy()[:, [2, 0]], f.numpy()[:, [0, 1]]], 0), 1)
    uniq, count = np.unique(e, axis=0, return_counts=True)
    assert (count == 2).all() and uniq.shape[0] == 30 * 4 ** level          # closed
    fv = v.double()[f]
    volume = float((fv[:, 0] * torch.cross(fv[:, 1], fv[:, 2], dim=1)).sum() / 6.0)
    assert 2.5 < volume < 4.0 / 3.0 * np.pi                                  # oriented outwards, inside the unit ball
    # every face on its own points away from the origin
    assert float(((fv[:, 0] + fv[:, 1] + fv[:, 2]) * torch.cross(fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0], dim=1)).sum(1).min()) > 0
    assert np.array_equal(m.edges_packed().numpy(), uniq) and int(m.num_edges_per_mesh()[0]) == uniq.shape[0]


def test_save_obj_round_trip(tmp_path):
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.io import load_obj, save_obj
    v, f = _ico(1)
    v = (v * np.float32(1.2345678)).astype(np.float32)
    path = str(tmp_path / "mesh.obj")
    save_obj(path, torch.from_numpy(v), torch.from_numpy(f))
    lines = open(path).read().splitlines()
    assert [ln.split()[0] for ln in lines] == ["v"] * 42 + ["f"] * 80 and lines[42].split()[1:] == [str(i + 1) for i in f[0]]
    rv, rf, _ = load_obj(path)
    assert torch.equal(rv, torch.from_numpy(v)) and torch.equal(rf.verts_idx, torch.from_numpy(f))
    buf = io.StringIO()
    save_obj(buf, torch.from_numpy(v), torch.from_numpy(f).float(), decimal_places=3)      # a file object, float faces
    buf.seek(0)
    rv, rf, _ = load_obj(buf)
    assert float((rv - torch.from_numpy(v)).abs().max()) <= 5.01e-4 and torch.equal(rf.verts_idx, torch.from_numpy(f))


def test_meshes_queries_and_float_faces():
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim import structures
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.structures import Meshes
    c = mesh_case("two-topologies")
    ms, _ = c.meshes(torch.device("cpu"))
    e = edges_of(c.fp)
    assert np.array_equal(ms.edges_packed().numpy(), e)
    assert ms.num_edges_per_mesh().tolist() == [120, 9 * 6 + 8 * 7 + 8 * 6]
    assert np.array_equal(ms.edges_packed_to_mesh_idx().numpy(), c.mesh_of_vert[e[:, 0]])
    assert ms.mesh_to_faces_packed_first_idx().tolist() == [0, 80]
    f2e = ms.faces_packed_to_edges_packed().numpy()
    for k, (i, j) in enumerate(((1, 2), (2, 0), (0, 1))):
        assert np.array_equal(e[f2e[:, k]], np.sort(c.fp[:, [i, j]], 1))
    v1, f1 = ms.get_mesh_verts_faces(1)
    assert v1.shape == (63, 3) and np.array_equal(f1.numpy(), c.faces[1])
    with pytest.raises(ValueError, match="range"):
        ms.get_mesh_verts_faces(2)
    quads, w = ms.normal_pairs_packed()
    want = pairs_of(c.fp)
    canon = lambda q: sorted((a, b, min(x, y), max(x, y)) for a, b, x, y in q.tolist())
    assert canon(quads.numpy()) == canon(want) and quads.dtype == torch.int64 and w.dtype == torch.float32
    # float faces, as fit_verts_to_mesh stores them, in a list; the tables are memoised on that tensor
    ff = torch.from_numpy(c.faces[0]).float()
    vv = torch.from_numpy(c.verts[0])
    ma = Meshes(verts=[vv], faces=[ff])
    qa = ma.normal_pairs_packed()[0]
    assert qa.shape == (120, 4) and ma.faces_packed_to_edges_packed().dtype == torch.int64
    mb = Meshes(verts=[vv + 1.0], faces=[ff])
    assert mb.normal_pairs_packed()[0] is qa and mb.num_edges_per_mesh() is ma.num_edges_per_mesh()
    ff.add_(0)                                                   # a new version of the tensor: not the old table
    assert Meshes(verts=[vv], faces=[ff]).normal_pairs_packed()[0] is not qa
    assert len(structures._TOPO_CACHE) <= 17


def test_chamfer_inputs_have_few_near_ties():
    for name in CHAMFER_NAMES:
        r = chamfer_reference(name)
        rows = r["tie_x"].size + r["tie_y"].size
        ties = int(r["tie_x"].sum() + r["tie_y"].sum())
        print("%s: %d near-tie rows of %d" % (name, ties, rows))
        assert ties <= TIE_SHARE * rows, name


@pytest.mark.parametrize("name", CHAMFER_NAMES)
def test_chamfer_host_path(name):
    check_chamfer(name + " host", chamfer_host(name), name)


def test_chamfer_duplicates_reference_and_host():
    """The float64 helper itself picks the lowest index among exact duplicates; a pair at distance 0 contributes a zero
    gradient (what the coincident points do receive comes from the other points that chose them: the reference's rows),
    and the host path's gradient is finite."""
    r = chamfer_reference("ties")
    assert r["ix"][0, 5] == 3 and r["iy"][0, 3] == 5 and r["iy"][0, 7] == 5 and r["iy"][0, 290] == 5
    assert r["ix"][0, 6] == r["ix"][0, 9]
    _, gx, gy = chamfer_host("ties")
    assert np.isfinite(gx).all() and np.isfinite(gy).all()
    assert not r["gy"][0, 7].any() and not r["gy"][0, 290].any()      # chosen by nobody, and at distance 0 from x[0, 5]
    assert not gy[0, 7].any() and not gy[0, 290].any()


def test_chamfer_reductions_and_weights():
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.loss import chamfer_distance
    c = chamfer_case("lengths")
    keep = [0, 1, 2]                                             # the clouds without a length of 0 (0 / 0 under "mean")
    x, y = torch.tensor(c.x[keep]), torch.tensor(c.y[keep])
    xl, yl, w = torch.tensor(c.xl[keep]), torch.tensor(c.yl[keep]), torch.tensor(c.w[keep])
    cx, cy = np.zeros(3), np.zeros(3)
    for n in range(3):
        a, b = c.x[n, :c.xl[n]].astype(np.float64), c.y[n, :c.yl[n]].astype(np.float64)
        cx[n], cy[n] = _nearest64(a, b)[1].sum(), _nearest64(b, a)[1].sum()
    for weights in (None, w):
        wn = np.ones(3) if weights is None else c.w[keep].astype(np.float64)
        for pr in ("mean", "sum"):
            px = cx * wn / (c.xl[keep] if pr == "mean" else 1.0)
            py = cy * wn / (c.yl[keep] if pr == "mean" else 1.0)
            for br in ("mean", "sum", None):
                want = px + py
                if br is not None:
                    want = want.sum() / ((wn.sum() if weights is not None else 3.0) if br == "mean" else 1.0)
                got, none = chamfer_distance(x, y, xl, yl, weights=weights, batch_reduction=br, point_reduction=pr)
                assert none is None
                np.testing.assert_allclose(got.numpy(), want, rtol=VALUE_RTOL, err_msg="%s %s %s" % (weights is not None, pr, br))
    # defaults: full lengths, mean / mean
    got, _ = chamfer_distance(torch.tensor(c.x[:1, :20]), torch.tensor(c.y[:1, :5]))
    a, b = c.x[0, :20].astype(np.float64), c.y[0, :5].astype(np.float64)
    np.testing.assert_allclose(got.item(), _nearest64(a, b)[1].mean() + _nearest64(b, a)[1].mean(), rtol=VALUE_RTOL)


@pytest.mark.parametrize("name,target", EDGE_RUNS)
def test_edge_loss_host_path(name, target):
    loss, grad = mesh_host(name, "edge", target)
    check_mesh_term("%s edge target %.1f host" % (name, target), loss, grad, name, "edge", target, host=False)


@pytest.mark.parametrize("name", NORMAL_RUNS)
def test_normal_consistency_host_path(name):
    """The float32 host path.  Gradient: the suite's rtol / atol (its relative L2 is printed: the GPU test's L2 bar is
    4 x that figure).  Value: the loss is the mean of 1 - cos over the pairs (the weights of a mesh sum to 1, the batch
    is divided by N); a float32 cos (three products and two adds per dot product, two norms, one division) is within
    16 eps of the exact one, so the mean is off by at most 16 eps absolute, i.e. 16 eps / value relative.  The measured
    error is printed: the GPU test's value bar is 4 x that."""
    loss, grad = mesh_host(name, "normal")
    ref_v, ref_g, keep = mesh_reference(name, "normal")
    bar = max(VALUE_RTOL, 16 * float(np.finfo(np.float32).eps) / abs(ref_v))
    print("%s normal host: value rel err %.2e (bar %.2e)" % (name, abs(loss - ref_v) / abs(ref_v), bar))
    np.testing.assert_allclose(loss, ref_v, rtol=bar, err_msg=name)
    assert np.isfinite(grad).all()
    check_grad(name + " normal host grad", grad, ref_g, keep, float("inf"))


def test_mesh_terms_special_cases():
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim import loss as L
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.structures import Meshes
    dev = torch.device("cpu")
    ms, _ = mesh_case("fan").meshes(dev)
    assert ms.normal_pairs_packed()[0].shape == (3, 4)                     # an edge in three faces: three pairs
    np.testing.assert_allclose(ms.normal_pairs_packed()[1].numpy(), [1 / 3.0] * 3, rtol=1e-7)
    ms, _ = mesh_case("no-shared-edge").meshes(dev)
    z = L.mesh_normal_consistency(ms)
    assert ms.normal_pairs_packed()[0].shape == (0, 4) and z.shape == (1,) and float(z.detach()) == 0.0 and z.requires_grad
    empty = Meshes(verts=[], faces=[])
    for fn in (L.mesh_edge_loss, L.mesh_normal_consistency):
        z = fn(empty)
        assert z.shape == (1,) and float(z.detach()) == 0.0 and z.requires_grad
    # the zero-length edge: finite, subgradient 0 (target 0.1: the term itself is not 0 there)
    _, grad = mesh_host("zero-edge", "edge", 0.1)
    assert np.isfinite(grad).all()
    assert len(mesh_reference("zero-edge", "normal")[2]) - int(mesh_reference("zero-edge", "normal")[2].sum()) >= 3


def test_sampling_deterministic_part():
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.ops import sample_points_from_faces
    c = mesh_case("two-topologies")
    rng = np.random.default_rng(4)
    S = 500
    idx = np.stack([rng.integers(0, 80, S), 80 + rng.integers(0, c.faces[1].shape[0], S)])
    u, v = rng.uniform(0, 1, (2, S)).astype(np.float32), rng.uniform(0, 1, (2, S)).astype(np.float32)
    verts = torch.tensor(c.vp, requires_grad=True)
    pts, nrm = sample_points_from_faces(verts, torch.from_numpy(c.fp).float(), torch.from_numpy(idx), torch.from_numpy(u),
                                        torch.from_numpy(v), return_normals=True)
    assert pts.shape == (2, S, 3) and nrm.shape == (2, S, 3)
    su = np.sqrt(u.astype(np.float64))
    w = np.stack([1 - su, su * (1 - v), su * v], -1)                          # [2,S,3]
    tri = c.vp.astype(np.float64)[c.fp[idx]]                                  # [2,S,3,3]
    want = (w[..., None] * tri).sum(2)
    assert float(np.abs(pts.detach().numpy() - want).max()) <= 1e-6           # every point reconstructs from its face
    n = np.cross(tri[:, :, 1] - tri[:, :, 0], tri[:, :, 2] - tri[:, :, 0])
    np.testing.assert_allclose(nrm.detach().numpy(), n / np.linalg.norm(n, axis=-1, keepdims=True), atol=1e-5)
    pts.sum().backward()                                                      # each vertex: the sum of its weights
    acc = np.zeros(c.P)
    np.add.at(acc, c.fp[idx].reshape(-1), w.reshape(-1))
    np.testing.assert_allclose(verts.grad.numpy(), np.repeat(acc[:, None], 3, 1), rtol=1e-5, atol=1e-6)


def test_sampling_drawn_part():
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.ops import sample_points_from_meshes
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.structures import Meshes
    # two faces in the plane z = 0 with areas 1 (x < 0) and 3 (x > 0)
    v = torch.tensor([[0, 0, 0], [-2, 0, 0], [0, 1, 0], [6, 0, 0.0]], requires_grad=True)
    f = torch.tensor([[0, 2, 1], [0, 3, 2]])
    torch.manual_seed(1234)
    S = 20000
    pts, nrm = sample_points_from_meshes(Meshes(verts=[v], faces=[f.float()]), S, return_normals=True)
    assert pts.shape == (1, S, 3) and pts.requires_grad
    share = float((pts[0, :, 0] < 0).float().mean())
    print("share of the small face: %.4f (0.25 +- %.4f)" % (share, 5 * np.sqrt(0.25 * 0.75 / S)))
    assert abs(share - 0.25) <= 0.0153
    p = pts.detach()[0]
    assert float(p[:, 2].abs().max()) == 0 and float(p[:, 1].min()) >= 0
    assert bool(((p[:, 0] >= -2 * (1 - p[:, 1]) - 1e-5) & (p[:, 0] <= 6 * (1 - p[:, 1]) + 1e-5)).all())   # inside the faces
    assert torch.equal(nrm[0], torch.tensor([0, 0, 1.0]).expand(S, 3))
    # a mesh without faces yields zeros; an empty batch is refused
    two = Meshes(verts=[v.detach(), v.detach()], faces=[f, f[:0]])
    out = sample_points_from_meshes(two, 7)
    assert out.shape == (2, 7, 3) and not out[1].any() and out[0].any()
    with pytest.raises(ValueError, match="Meshes are empty."):
        sample_points_from_meshes(Meshes(verts=[], faces=[]), 5)
    assert sample_points_from_meshes(Meshes(verts=[v], faces=[f])).shape == (1, 10000, 3)


def test_refusals():
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.loss import chamfer_distance
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.utils import ico_sphere
    x, y = torch.zeros(2, 4, 3), torch.zeros(2, 5, 3)
    with pytest.raises(ValueError, match="x_normals"):
        chamfer_distance(x, y, x_normals=torch.zeros(2, 4, 3))
    with pytest.raises(ValueError, match="y_normals"):
        chamfer_distance(x, y, y_normals=torch.zeros(2, 5, 3))
    with pytest.raises(ValueError, match="x must have shape"):
        chamfer_distance(torch.zeros(2, 4, 2), y)
    with pytest.raises(ValueError, match="y must have shape"):
        chamfer_distance(x, torch.zeros(2, 5, 4))
    with pytest.raises(ValueError, match="y must have shape"):
        chamfer_distance(x, torch.zeros(3, 5, 3))
    with pytest.raises(ValueError, match="batch_reduction"):
        chamfer_distance(x, y, batch_reduction="max")
    with pytest.raises(ValueError, match="point_reduction"):
        chamfer_distance(x, y, point_reduction="none")
    with pytest.raises(ValueError, match="x_lengths"):
        chamfer_distance(x, y, x_lengths=torch.tensor([1, 2, 3]))
    with pytest.raises(ValueError, match="weights"):
        chamfer_distance(x, y, weights=torch.ones(3))
    with pytest.raises(ValueError, match="level"):
        ico_sphere(-1)
