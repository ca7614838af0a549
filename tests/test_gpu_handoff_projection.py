"""GPU: NeuralRenderer.project_points served from the renderer's last silhouette render (nnutils/nmr.py `_LAST_PROJ`,
ops/render.py `_proj_key` / `_proj_serves`) against the plain path it must equal, `ops.project_xy(verts, cams)` on tensors
of the autograd identity the caller passed -- for every way a caller can present the render's storage again: detached,
under no_grad, as a new leaf, after the storage has been recycled, across a hipGraph capture.  A mistake here raises
nothing; it gives a gradient that is missing, goes to the wrong tensor, or a projection of other geometry.

Forward: torch.equal (test_gpu_dropin.py demands equal bits of the hand-off).  Gradients: that test's bound,
<= 2e-6 * max|ref|.  Scene: horse, N = 4, H = 64 (test_gpu_dropin.py's)."""
import gc
import itertools

import pytest
import torch

import handoffs as HO

pytestmark = pytest.mark.gpu

N, H = 4, 64
PRESENT = ("attached", "detached")
MODES = ("grad", "no_grad")
IDENTITIES = [(v, c, m) for v in PRESENT for c in PRESENT for m in MODES]       # (verts, cams, grad mode)
WRAPPERS = ("forward", "forward_silhouette_losses")


def _d():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def I(meshes):
    return HO.scene(meshes, _d(), "horse", N, H, 2, 41)


def _mode(m):
    return torch.enable_grad() if m == "grad" else torch.no_grad()


def _present(t, how):
    return t if how == "attached" else t.detach()


def _render(ren, wrapper, I, v, c):
    if wrapper == "forward":
        return ren(v, I["faces"], c)
    return ren.forward_silhouette_losses(v, I["faces"], c, I["gt"], I["edt"])


def _profiled(fn):
    """fn() with the kernel profile on -> (its result, {kernel: (ms, launches)})."""
    from acfm_video_3d_reconstruction_amd import _lib
    lib = _lib.lib()
    torch.cuda.synchronize()
    lib.acfm_prof_enable(1)
    try:
        out = fn()
        torch.cuda.synchronize()
        ran = _lib.prof_collect()
    finally:
        lib.acfm_prof_enable(0)
    return out, ran


def _cell(I, wrapper, at_render, at_project):
    """One cell: render with the leaves presented as `at_render`, project with them presented as `at_project`; the plain
    call on leaves of its own, presented as `at_project`.  Asserts everything the issue asks of a cell."""
    from acfm_video_3d_reconstruction_amd import ops
    from acfm_video_3d_reconstruction_amd.nnutils.nmr import NeuralRenderer
    d = _d()
    ren = NeuralRenderer(H)
    tv, tc = HO.leaves(I, d)
    rv, rc = HO.leaves(I, d)
    w = torch.randn(N, I["verts"].shape[1], 2, device=d, generator=torch.Generator(device=d).manual_seed(5))
    with _mode(at_render[2]):
        out = _render(ren, wrapper, I, _present(tv, at_render[0]), _present(tc, at_render[1]))
    with _mode(at_project[2]):
        got, ran = _profiled(lambda: ren.project_points(_present(tv, at_project[0]), _present(tc, at_project[1])))
        want = ops.project_xy(_present(rv, at_project[0]), _present(rc, at_project[1]))
    what = (wrapper, at_render, at_project)
    assert torch.equal(got, want), what
    assert got.requires_grad == want.requires_grad and (got.grad_fn is None) == (want.grad_fn is None), what
    if want.requires_grad:
        g, g_raw = HO.grads((got * w).sum(), [tv, tc])
        r, r_raw = HO.grads((want * w).sum(), [rv, rc])
        for name, a, b, a_raw, b_raw in zip(("verts", "cams"), g, r, g_raw, r_raw):
            assert (a_raw is None) == (b_raw is None), what + (name, "the plain call's gradient is %s"
                                                               % ("None" if b_raw is None else "there"))
            if b_raw is not None:
                ok, fig = HO.close(a, b, 2e-6)
                assert ok, what + (name,) + fig
    else:
        assert not got.requires_grad
    if at_render != at_project:
        assert "k_project" in ran, what + ("served from a render of another autograd identity", ran)
    if at_render == at_project == ("attached", "attached", "grad"):
        assert "k_project" not in ran, what + ("the hand-off is no longer taken", ran)
    del out


@pytest.mark.parametrize("at_project", IDENTITIES, ids="-".join)
@pytest.mark.parametrize("at_render", IDENTITIES, ids="-".join)
def test_autograd_identity_matrix(I, at_render, at_project):
    """Render-time and projection-time (verts, cams) from {attached, .detach()} each x {grad mode, no_grad}: the result's
    requires_grad / grad_fn and the gradient to each leaf (None where the plain call's is None) are the plain call's;
    every cell that differs from the render's identity runs k_project; the all-attached cell does NOT (the hand-off
    is still taken).  `.detach()` shares address, version, shape and dtype with its source."""
    _cell(I, "forward", at_render, at_project)


A, D = "attached", "detached"
DEFECT_CELLS = {
    "1a-render-detached": ((D, D, "grad"), (A, A, "grad")),
    "1a-render-no_grad": ((A, A, "no_grad"), (A, A, "grad")),
    "1b-project-detached": ((A, A, "grad"), (D, D, "grad")),
    "1c-cams-detached-at-render": ((A, D, "grad"), (A, A, "grad")),
    "control-all-attached": ((A, A, "grad"), (A, A, "grad")),
}


@pytest.mark.parametrize("cell", sorted(DEFECT_CELLS))
@pytest.mark.parametrize("wrapper", WRAPPERS)
def test_defect_cells_through_both_wrappers(I, wrapper, cell):
    """The cells in which a gradient was dropped (1a), invented (1b) or lost for the cameras (1c), and the control,
    through NeuralRenderer.forward and through forward_silhouette_losses."""
    _cell(I, wrapper, *DEFECT_CELLS[cell])


def test_a_new_leaf_on_the_render_storage_gets_its_own_gradient(I):
    """`verts.detach().requires_grad_()` is another place in the graph on the same address, version and requires_grad:
    its projection must back-propagate to IT, not to the tensor that was rendered."""
    from acfm_video_3d_reconstruction_amd import ops
    from acfm_video_3d_reconstruction_amd.nnutils.nmr import NeuralRenderer
    d = _d()
    ren = NeuralRenderer(H)
    tv, tc = HO.leaves(I, d)
    ren(tv, I["faces"], tc)
    nv = tv.detach().requires_grad_(True)
    assert nv.data_ptr() == tv.data_ptr() and nv._version == tv._version
    got, ran = _profiled(lambda: ren.project_points(nv, tc))
    assert "k_project" in ran
    w = torch.randn(N, I["verts"].shape[1], 2, device=d)
    (g_new, g_old, g_c), raw = HO.grads((got * w).sum(), [nv, tv, tc])
    assert raw[1] is None and raw[0] is not None
    rv, rc = HO.leaves(I, d)
    (r_v, r_c), _ = HO.grads((ops.project_xy(rv, rc) * w).sum(), [rv, rc])
    assert HO.close(g_new, r_v, 2e-6)[0] and HO.close(g_c, r_c, 2e-6)[0]


@pytest.mark.parametrize("how", ["share_setup_off", "second_renderer_between"])
def test_recycled_address(I, how):
    """Defect 2: after a no_grad render nothing but the caches holds the vertices.  With the device's _SETUP entry gone
    too (sharing off, or another renderer -- the trainer keeps two -- rendered in between) the storage could be freed
    and a new tensor of the same shape land on the address at version 0: project_points must give the projection of
    the NEW values.  The entry keeps its inputs alive now.  Both halves are asserted: while the entry is there no new
    tensor gets the address and new values are projected by the kernel; once the entry is gone the address does
    come back (the helper fails the test if it does not), and the projection still is the plain one."""
    from acfm_video_3d_reconstruction_amd import ops
    from acfm_video_3d_reconstruction_amd.nnutils.nmr import NeuralRenderer
    d = _d()
    ren, other = NeuralRenderer(H), NeuralRenderer(H)
    cams = torch.tensor(I["cams"], device=d)
    base = torch.tensor(I["verts"], device=d)
    make = lambda: base * 1.25                                   # (one allocation, version 0: nothing else takes the freed block)
    # the allocator does recycle here: a dropped tensor's address comes back for an equal-sized request
    probe = make()
    HO.dropping(probe)
    del probe
    again = HO.recycled(make)
    del again
    from acfm_video_3d_reconstruction_amd.nnutils import nmr
    with HO.plain(share=(how == "share_setup_off")):
        # (neighbours in use on both sides: the freed block is not merged into a larger one, and an equal-sized request
        # gets it back)
        before = make()
        verts = base.clone()
        after = make()
        with torch.no_grad():
            ren(verts, I["faces"], cams)
            if how == "second_renderer_between":
                other(base, I["faces"], cams)               # replaces the device's _SETUP entry
        HO.dropping(verts)
        del verts
        gc.collect()
        # 1. while the renderer's entry is there it holds the vertices: no new tensor lands on their address, and a
        #    new tensor of other values is projected by the kernel
        news = HO.pinned(make, attempts=8)
        assert news[0]._version == 0
        with torch.no_grad():
            got = ren.project_points(news[0], cams)
            want = ops.project_xy(news[0], cams)
        assert torch.equal(got, want)
        assert not torch.equal(want, ops.project_xy(base, cams))  # (the previous geometry's projection would have shown)
        # 2. the entry was the last holder: without it the address does come back (so 1. showed something)
        del news, got, want
        nmr._LAST_PROJ.pop(ren, None)
        gc.collect()
        new = HO.recycled(make, attempts=12)             # (the eight blocks of 1. are free again as well)
        assert new._version == 0
        with torch.no_grad():
            assert torch.equal(ren.project_points(new, cams), ops.project_xy(new, cams))
        del before, after


def test_capture_boundary(I):
    """Defect 3: a projection made inside a hipGraph capture lives in the graph's pool and is rewritten by every replay:
    it must not be handed out after the capture.  An eager project_points behind a replay is the caller's own tensor
    (a later replay leaves it alone) and equals the plain call."""
    from acfm_video_3d_reconstruction_amd import ops
    from acfm_video_3d_reconstruction_amd.nnutils.nmr import NeuralRenderer
    d = _d()
    ren = NeuralRenderer(H)
    sv, sc = torch.tensor(I["verts"], device=d), torch.tensor(I["cams"], device=d)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        ren(sv, I["faces"], sc)                                   # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g), torch.no_grad():
        mask, _ = ren(sv, I["faces"], sc)
    ops.graph_replay(g)
    torch.cuda.synchronize()
    with torch.no_grad():
        p = ren.project_points(sv, sc)
        p0 = p.clone()
        assert torch.equal(p, ops.project_xy(sv, sc))
        sv.mul_(0.9).add_(0.02)
        ops.graph_replay(g)
        torch.cuda.synchronize()
        assert torch.equal(p, p0), "a replay rewrote the projection the caller holds"
        assert torch.equal(ren.project_points(sv, sc), ops.project_xy(sv, sc))
        assert not torch.equal(ops.project_xy(sv, sc), p0)
    del g, mask


def test_entry_keeps_its_inputs_and_is_dropped_with_the_hand_off(I):
    """The entry holds (verts, cams) the way _Setup.inputs does -- while it is there their addresses cannot be recycled --
    and lets go of them when the projection has been handed out or another render replaced it."""
    import weakref
    from acfm_video_3d_reconstruction_amd.nnutils import nmr
    d = _d()
    ren = nmr.NeuralRenderer(H)
    cams = torch.tensor(I["cams"], device=d)
    with HO.plain(share=True), torch.no_grad():
        verts = torch.tensor(I["verts"], device=d)
        alive = weakref.ref(verts)
        p2f = ren(verts, I["faces"], cams)[1]
        del verts, p2f
        gc.collect()
        assert alive() is not None and nmr._LAST_PROJ[ren][2][0] is alive()
        ren.project_points(alive(), cams)                         # handed out: the entry goes, and its hold with it
        gc.collect()
        assert ren not in nmr._LAST_PROJ and alive() is None
