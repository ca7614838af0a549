"""CPU: the C oracle's rasteriser (oracle/acfm_oracle.c calls itself "parity unpinned" there) against a float64
restatement of its accept / reject rules on the hand-built scenes of tests/raster_scenes.py -- exact depth ties at
the truncation to K, pixel centres on edges and vertices, depths that cross zero, areas either side of kEps, the
degenerate-edge branch, all-degenerate and off-screen meshes in a batch, boxes on pixel, block and tile boundaries, a
face over the whole image.  No pixel is left out: every decision quantity of every scene is either exactly at its
threshold (in float32 as well) or further than 1e-5 relative (1e-9 absolute for the distance) from it, which the
test asserts and prints per scene."""
import numpy as np
import pytest

import raster_scenes as S
from oracle import oracle as O

SCENES = S.cpu_scenes()
IDS = [s["name"] for s, _ in SCENES]


def _sets(p2f, n, F):
    """pix_to_face [H,H,K] of mesh n -> membership [H,H,F]."""
    H = p2f.shape[0]
    m = np.zeros((H, H, F + 1), bool)
    loc = np.where(p2f >= 0, p2f - n * F, F)
    np.put_along_axis(m, loc, True, -1)
    return m[..., :F]


@pytest.mark.parametrize("scene,Ks", SCENES, ids=IDS)
def test_oracle_accepts_what_the_definition_accepts(scene, Ks):
    fv, H, N, F = S.face_verts(scene), scene["H"], scene["N"], scene["F"]
    worst = {}
    for blur in (0.0, S.SIL_BLUR):
        for clip in (False, True):
            for K in Ks:
                m = S.margins(fv, H, K, blur, clip, N)
                assert not S.check_margins(m), (blur, clip, K, S.check_margins(m))
                for k, (lo, n0, _) in m.items():
                    w = worst.setdefault(k, [np.inf, 0])
                    w[0], w[1] = min(w[0], lo), max(w[1], n0)
                ref = S.definition(fv, H, K, blur, clip, N)
                p2f = O.rasterize(fv, N, H, K, blur, clip_bary=clip)[0]
                for n in range(N):
                    got = _sets(p2f[n], n, F)
                    cnt = ref["accepted"][n].sum(-1)
                    np.testing.assert_array_equal((p2f[n] >= 0).sum(-1), np.minimum(cnt, K))
                    # at most K candidates: the accepted set; more: the K nearest -- where the depths either side of the
                    # cut are equal (an exact tie, checked in float32 by margins) the lower ids
                    np.testing.assert_array_equal(got, ref["kept"][n])
    print("%s: smallest margins (quantities exactly at their threshold): %s" % (
        scene["name"], ", ".join("%s %.2g (%d)" % (k, v[0], v[1]) for k, v in sorted(worst.items()))))


@pytest.mark.parametrize("K", [1, 2, 4, 8, 10, 20, 32])
def test_exact_ties_keep_the_lowest_ids(K):
    for M in S.dup_stack_cases(K):
        sc = S.dup_stack(K, M)
        fv, H = S.face_verts(sc), sc["H"]
        dup = np.array(sc["dup_ids"])
        assert len(dup) == M
        p2f, zbuf, _, _ = O.rasterize(fv, 1, H, K, S.SIL_BLUR)
        got = _sets(p2f[0], 0, sc["F"])
        n_dup = got[..., dup].sum(-1)
        full = (p2f[0] >= 0).all(-1) & (n_dup > 0)
        assert full.sum() > 10
        if M >= K:
            assert (n_dup[full] < M).any() or M == K          # the tie group is cut somewhere
        for y, x in zip(*np.nonzero(n_dup > 0)):
            k = n_dup[y, x]
            assert got[y, x, dup[:k]].all(), (y, x)           # the kept copies are the k lowest ids
            zs = zbuf[0, y, x][np.isin(p2f[0, y, x], dup)]
            assert (zs == zs[0]).all()                        # and they are exact ties
        if K > 2:
            near = (n_dup > 0) & (n_dup < min(M, K))          # nearer faces in front: the group straddles slot K - 1
            assert near.any() or M < K


def test_one_ulp_copies_are_not_ties():
    """Reversed and rotated vertex orders of one face give depths 1 ulp apart in float32: their order is the C oracle's,
    not exact arithmetic's (the GPU test compares them with the oracle only)."""
    sc = S.dup_stack(4, 6, ulp=True)
    _, zbuf, _, _ = O.rasterize(S.face_verts(sc), 1, sc["H"], 8, 0.0)
    z = zbuf[0][(zbuf[0] >= 0).sum(-1) >= 6]
    assert len(z) > 10
    d = np.diff(np.sort(z[:, :8], -1), axis=-1)
    assert ((d > 0) & (d < 1e-6)).any()


def test_shared_edge_known_answers():
    sc = S.shared_edge()
    fv, H = S.face_verts(sc), sc["H"]
    p0, _, _, _ = O.rasterize(fv, 1, H, 4, 0.0)
    p1, _, _, d1 = O.rasterize(fv, 1, H, 4, S.SIL_BLUR)
    for (r, u), pair in sc["edge_faces"].items():
        assert not np.isin(p0[0, r, u], pair).any(), (r, u)             # on the edge: neither face at blur 0
        for f in pair:                                                    # both, at distance exactly 0, with blur
            k = np.flatnonzero(p1[0, r, u] == f)
            assert len(k) == 1 and d1[0, r, u, k[0]] == 0.0, (r, u, f)
    assert (p0[0, 3:10, 5, 0] == 0).all() and (p0[0, 3:10, 7, 0] == 1).all()   # and either side belongs to its face


def test_z_cross_accepts_the_half_plane():
    sc = S.z_cross()
    fv, H = S.face_verts(sc), sc["H"]
    r, u = np.meshgrid(np.arange(H), np.arange(H), indexing="ij")
    for blur in (0.0, S.SIL_BLUR):
        p2f, zbuf, _, _ = O.rasterize(fv, 1, H, 4, blur, clip_bary=False)
        has = [(p2f[0] == f).any(-1) for f in range(2)]
        q = S._cached(fv[:sc["F"]], H, blur, False)[0]
        geo = q["inbox"] & (q["inside"] | (q["d"] < q["blur"]))          # inside the face, or within blur of it
        # face 0: pz = 4 b1 - 1 >= 0 <=> row <= 22; face 1: <=> u + r <= 24
        cover = [geo[..., f] for f in range(2)]
        np.testing.assert_array_equal(has[0], cover[0] & (r <= 22))
        np.testing.assert_array_equal(has[1], cover[1] & (u + r <= 24))
        assert has[0][22].sum() > 10 and (u + r == 24)[has[1]].sum() > 5       # the pz == 0 pixels are kept
        assert (zbuf[0][(p2f[0] == 0) & (r == 22)[..., None]] == 0.0).all()


@pytest.mark.parametrize("H", [64, 40])
def test_box_scene_puts_box_sides_on_pixel_centres(H):
    """What box_on_boundaries is for: sides of face boxes, without and with sqrt(blur), that ARE pixel-centre columns
    and rows in float32 (and pixel, block and coarse-tile boundaries between them), on all four sides of a box."""
    sc = S.box_on_boundaries(H)
    fv = S.face_verts(sc)
    c = S.ndc_of(np.arange(H), H)
    for blur, least in ((0.0, 6), (S.SIL_BLUR, 4)):
        box = S._eval(fv, H, blur, False, np.float32)["box"]
        for side in box:                                   # x min, x max, y min, y max
            assert np.isin(side, c).sum() >= least, (blur, np.isin(side, c).sum())
    corners = fv[:48, 0, :2]                               # the right-angle corners: the anchors, in pixel units
    u = ((1.0 - corners.astype(np.float64)) * H - 1.0) / 2.0
    for want in (-0.5, 0.0, 7.5, 8.0, 15.5, 16.0, H - 1.0, H - 0.5):
        assert (np.abs(u - want) < 1e-4).any(), want
