"""Hand-built raster scenes and a float64 definition of the rasteriser's accept / reject rules.

Every builder returns a dict: ndc float32 [N,V,3] = (NDC x, NDC y, view z), faces int64 [F,3] or [N,F,3], H, blur (the
blur the scene is about: SIL_BLUR or 0.0), name, and flags for what the scene is about.  sil_inputs(scene) gives the
same scene as (verts, cams) for the silhouette and texture entry points.

Coordinates are written in PIXEL units and turned into NDC by ndc_of(u, H) = 1 - (2u + 1) / H: an integer u is the
centre of pixel u (the rasteriser's own float32 expression), u + 0.5 the boundary between pixels u and u + 1.  With H a
power of two and u a multiple of 1/4 every coordinate is dyadic and every edge function of a pixel centre is exact in
float32, so "the pixel centre is ON the edge" is an exact statement on both sides of a comparison.

definition() restates oracle_rasterize (oracle/acfm_oracle.c) in float64 numpy; margins() measures how far every
decision quantity of a scene is from its threshold, so that float32 and float64 agree on every pixel by reasoning:
the float32 rounding error of a quantity is a few units of 6e-8 times the magnitude of its terms, a quantity further
than 1e-5 of that magnitude from its threshold is decided alike in both, and a quantity exactly AT its threshold is
checked to be there in float32 as well."""
import math

import numpy as np

SIL_BLUR = math.log(1.0 / 1e-4 - 1.0) * 1e-4
EYE_Z = 2.732
K_EPS = np.float32(1e-8)


def ndc_of(u, H):
    """Pixel coordinate (integer = pixel centre) -> NDC, float32, as pix_to_ndc(H - 1 - u, H) computes it."""
    u = np.asarray(u, np.float64)
    return np.float32(-1.0) + (np.float32(2.0) * (H - 1 - u).astype(np.float32) + np.float32(1.0)) / np.float32(H)


def _tri(H, p0, p1, p2, z):
    """One face from three (column u, row r) pixel coordinates; z a number or three."""
    z = np.broadcast_to(np.asarray(z, np.float32), (3,))
    return np.array([[ndc_of(p[0], H), ndc_of(p[1], H), z[i]] for i, p in enumerate((p0, p1, p2))], np.float32)


def _scene(name, meshes, H, blur, **flags):
    """meshes: a list (one entry per mesh) of lists of [3,3] faces.  Every face gets vertices of its own (V = 3 F), one
    further vertex is referenced by no face, and shorter meshes are padded with repeated-index faces (0, 0, 0)."""
    N, F = len(meshes), max(max(len(m) for m in meshes), 1)
    ndc = np.zeros((N, 3 * F + 1, 3), np.float32)
    ndc[:, -1] = (0.25, -0.25, 1.0)
    faces = np.zeros((N, F, 3), np.int64)
    for n, m in enumerate(meshes):
        for f, t in enumerate(m):
            ndc[n, 3 * f:3 * f + 3] = t
            faces[n, f] = (3 * f, 3 * f + 1, 3 * f + 2)
    if N == 1:
        faces = faces[0]
    return dict(name=name, ndc=ndc, faces=faces, H=H, blur=blur, N=N, F=F, unreferenced=3 * F, **flags)


def face_verts(scene):
    """[N*F,3,3] packed, as oracle.face_verts_of."""
    ndc, f = scene["ndc"], scene["faces"]
    N = ndc.shape[0]
    if f.ndim == 2:
        f = np.broadcast_to(f, (N,) + f.shape)
    return np.ascontiguousarray(ndc[np.arange(N)[:, None, None], f].reshape(-1, 3, 3))


def sil_inputs(scene):
    """(verts [N,V,3], cams [N,7]) whose silhouette / texture camera chain (identity camera, x and y negated, z + 2.732)
    renders the scene; the oracle goes through the same chain, so z need not round-trip exactly."""
    ndc = scene["ndc"]
    verts = np.stack([-ndc[..., 0], -ndc[..., 1], ndc[..., 2] - np.float32(EYE_Z)], -1).astype(np.float32)
    cams = np.tile(np.array([1, 0, 0, 1, 0, 0, 0], np.float32), (ndc.shape[0], 1))
    return verts, cams


# ------------------------------------------------------------------------------------------------ face lists
def _shared_edge_faces(H):
    """Two faces share the edge column 6, rows 2..10 (through pixel centres, 8 pixels long: the projection parameter
    of point_line_dist is k/8, exact); two more share the edge row 13, columns 2..10; the end points are pixel centres."""
    return [_tri(H, (6, 2), (6, 10), (1.5, 6), 1.0), _tri(H, (6, 2), (12.5, 6), (6, 10), 1.5),
            _tri(H, (2, 13), (10, 13), (7.5, 15.25), 2.0), _tri(H, (2, 13), (7.5, 11.75), (10, 13), 2.5)]


_ORDERS = ((0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1), (2, 1, 0), (1, 0, 2))


def _dup_stack_faces(H, K, M, ulp=False):
    """M copies of one face (depth 1 .. 2 over its vertices) among `near` nearer faces that cover part of it and two
    farther ones: at the pixels all of them cover the tie group sits in slots near .. near + M - 1.  ids interleave
    the three kinds.  ulp: the copies run through the six vertex orders instead (depths 1 ulp apart in float32)."""
    base = _tri(H, (1.5, 1.5), (14.5, 3.5), (5.5, 14.5), (1.0, 1.5, 2.0))
    near = 0 if K == 1 else 1 if K == 2 else 2
    kinds = ["dup"] * M
    others = ["near%d" % i for i in range(near)] + ["far0", "far1"]
    step = max(1, M // (len(others) + 1))
    for i, o in enumerate(others):
        kinds.insert(min(len(kinds), (i + 1) * step + i - (1 if i % 2 else 0)), o)
    if M > 1:
        kinds.insert(0, kinds.pop(kinds.index("far0")))          # a farther face has the lowest id of all
    out, c = [], 0
    for k in kinds:
        if k == "dup":
            out.append(base[list(_ORDERS[c % 6])] if ulp else base.copy())
            c += 1
        elif k.startswith("near"):
            i = int(k[4:])
            out.append(_tri(H, (0.5 + 3 * i, 0.5), (15.5, 2.5 + 2 * i), (3.5, 9.25 + 3 * i), 0.25 + 0.25 * i))
        else:
            i = int(k[3:])
            out.append(_tri(H, (0.5, 0.5 + i), (15.5, 1.5), (8.5 - 4 * i, 15.5), (3.0 + i, 3.5, 4.0)))
    return out


def _z_cross_faces(H):
    """Vertex depths (-1, 3, -1): unclipped pz = 4 b1 - 1.  Face 0: b1 = 1/4 along row 22 (pixel centres); face 1: along
    the diagonal u + r = 24 (through pixel centres).  Both have area 2 (a power of two, and area + kEps == area in
    float32): barycentrics and pz are exact, pz == 0 exactly on those lines.  A plain face lies behind both."""
    assert H == 32
    return [_tri(H, (0, 26), (16, 10), (32, 26), (-1.0, 3.0, -1.0)), _tri(H, (8, 24), (0, 0), (24, 8), (-1.0, 3.0, -1.0)),
            _tri(H, (-2.5, -1.5), (34.5, 3.5), (13.5, 35.5), 5.0)]


def _field_faces(H, count, seed, z0=1.0):
    """`count` small faces on the quarter-pixel grid (dyadic: every edge function is exact), depths z0 + 0.01 i."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        c = rng.integers(0, 4 * H, 2) / 4.0
        d = rng.integers(-20, 21, (3, 2)) / 4.0
        out.append(_tri(H, c + d[0], c + d[1], c + d[2], z0 + 0.01 * i))
    return out


def _giant_face(top=64.0, z=3.0):
    """Covers the image: the square [-1, 1]^2 lies inside (-64, -64), (64, -64), (0, top) for any top >= 64."""
    return np.array([[-64.0, -64.0, z], [64.0, -64.0, z], [0.0, top, z]], np.float32)


# ------------------------------------------------------------------------------------------------ scenes
def shared_edge(H=16):
    """-> edge_faces: (row, column) of every pixel centre on a shared edge -> the two faces that share it."""
    return _scene("shared_edge", [_shared_edge_faces(H)], H, SIL_BLUR,
                  edge_faces={(r, 6): (0, 1) for r in range(2, 11)} | {(13, u): (2, 3) for u in range(2, 11)})


def dup_stack(K, M, ulp=False, H=16):
    faces = _dup_stack_faces(H, K, M, ulp)
    base = _tri(H, (1.5, 1.5), (14.5, 3.5), (5.5, 14.5), (1.0, 1.5, 2.0))
    key = sorted(map(tuple, base.tolist()))
    ids = [i for i, t in enumerate(faces) if sorted(map(tuple, t.tolist())) == key]
    return _scene("dup_stack[K=%d,M=%d%s]" % (K, M, ",ulp" if ulp else ""), [faces], H, SIL_BLUR, dup_ids=ids, ulp=ulp, K=K, M=M)


def dup_stack_cases(K):
    """M below, at and above K."""
    return [M for M in (K - 1, K, K + 1, K + 5) if M >= 1]


def z_cross():
    return _scene("z_cross", [_z_cross_faces(32)], 32, SIL_BLUR)


def area_eps():
    """Tiny faces at the image centre (a corner between four pixels, 2 / H^2 < blur away from their centres) with
    |area| = kEps / 2, kEps exactly (a * b with a = kEps * 2^13, b = 2^-13) and 2 kEps, both signs, in front of a normal
    face.  Only the 2 kEps pair is not degenerate; at blur 0 none of them covers a pixel centre."""
    H = 64
    b = np.float32(2.0 ** -13)
    faces = []
    for i, mult in enumerate((0.5, 1.0, 2.0)):
        a = np.float32(np.float32(K_EPS * np.float32(mult)) * np.float32(2.0 ** 13))
        z = 1.0 + 0.125 * i
        faces.append(np.array([[0, 0, z], [a, 0, z], [0, b, z]], np.float32))            # area = -a b
        faces.append(np.array([[0, 0, z + 0.0625], [0, b, z + 0.0625], [a, 0, z + 0.0625]], np.float32))   # +a b
    faces.insert(3, _tri(H, (20.5, 20.5), (44.5, 24.5), (30.5, 45.5), 2.0))
    return _scene("area_eps", [faces], H, SIL_BLUR, tiny_ids=[0, 1, 2, 4, 5, 6], live_tiny=[5, 6])


def short_edge():
    """(0, 0), (6e-5, 0), (0, 0.9): l2 of the first edge is 3.6e-9 <= kEps (point_line_dist's degenerate branch, the
    distance to the edge's END point) on a face of area 5.4e-5; the four pixels around the image centre lie within blur of
    that edge.  A mirrored copy has the short edge as its third edge; a normal face lies elsewhere."""
    H = 64
    s = np.float32(6e-5)
    faces = [np.array([[0, 0, 1.0], [s, 0, 1.0], [0, 0.9, 1.5]], np.float32),
             np.array([[0.5, -0.9, 2.0], [0.5, 0.0, 1.25], [0.5 + s, 0.0, 1.25]], np.float32),
             _tri(H, (40.5, 36.5), (60.5, 40.5), (47.5, 58.5), 1.75)]
    return _scene("short_edge", [faces], H, SIL_BLUR)


def all_degenerate_mesh(N=8):
    """A batch at H = 32: mesh 1 holds zero-area faces only (collinear and repeated vertices), mesh 3 lies wholly
    off-screen, the others hold other scenes; shorter meshes are padded with repeated-index faces."""
    H = 32
    line = [_tri(H, (2, 2), (10, 10), (18, 18), 1.0), _tri(H, (4, 20), (4, 20), (20, 6), 1.0),
            _tri(H, (3, 9), (9, 9), (27, 9), 2.0)]
    off = [np.array([[3.0, 0.5, 1.0], [4.0, 0.25, 1.0], [3.5, 1.5, 1.0]], np.float32),
           np.array([[-0.5, -3.0, 1.0], [0.5, -2.0, 1.0], [0.0, -4.5, 1.0]], np.float32)]
    meshes = [_shared_edge_faces(H), line, _dup_stack_faces(H, 4, 5), off, _z_cross_faces(H),
              _field_faces(H, 40, 5), [_giant_face()] + _field_faces(H, 12, 6), _dup_stack_faces(H, 8, 9)][:N]
    return _scene("all_degenerate_mesh[N=%d]" % N, meshes, H, SIL_BLUR, empty_meshes=[1, 3])


def _margin_anchor(c, margin, sign):
    """float32 x with fl(x + sign * margin) == c exactly: a vertex whose blur-expanded box side is the pixel centre c."""
    x = np.float32(c - sign * margin)
    for _ in range(8):
        got = np.float32(x + np.float32(sign) * margin)
        if got == c:
            return x
        x = np.nextafter(x, np.float32(np.inf if got < c else -np.inf), dtype=np.float32)
    return None          # x and c lie in different binades: x moves in steps of 2 ulp(c)


def box_on_boundaries(H=64):
    """Right triangles (legs 5 and 4.125 pixels: the hypotenuse meets no pixel centre) whose right-angle corner, and so two
    sides of the box, sits on a pixel centre, on a pixel boundary, on multiples of 8 pixels (raster blocks), of 16 (the
    coarse tiles, CTILE of csrc/acfm_common.h) and on the image border, legs pointing all four ways.  Then pointed faces
    whose box side WITH sqrt(blur) is exactly a pixel-centre column or row: the vertex sits half a pixel off the rows,
    so that no pixel of that column is at distance sqrt(blur) from it."""
    last = H - 1
    anchors = [-0.5, 0, 7, 7.5, 8, 15.5, 16, 31.5, 32, last - 7.5, last, last + 0.5]
    faces = []
    for i, a in enumerate(anchors):
        a2 = anchors[(i * 5 + 3) % len(anchors)]
        for j, (sx, sy) in enumerate(((1, 1), (-1, 1), (1, -1), (-1, -1))):
            faces.append(_tri(H, (a, a2), (a + 5 * sx, a2), (a, a2 + 4.125 * sy), 1.0 + 0.01 * (4 * i + j)))
    margin = np.float32(np.sqrt(np.float32(SIL_BLUR)))
    cols = [u for u in range(7, H - 7) if all(_margin_anchor(ndc_of(u, H), margin, s) is not None for s in (1, -1))]
    cols = [cols[0]] + [u for u in cols if u % 8 in (0, 7)][:3]      # block-boundary columns among them
    assert len(cols) == 4
    for i, (u, r) in enumerate(zip(cols, (20.5, 28.5, 11.5, 3.5))):
        for sign in (1, -1):                                         # the box's max side, then its min side
            z = 3.0 + 0.01 * (2 * i + (sign < 0))
            x = y = _margin_anchor(ndc_of(u, H), margin, sign)
            xs, ys = float(ndc_of(u + 4.25 * sign, H)), float(ndc_of(r, H))
            faces.append(np.array([[x, ys, z], [xs, float(ndc_of(r - 2.25, H)), z], [xs, float(ndc_of(r + 2.75, H)), z]], np.float32))
            faces.append(np.array([[ys, y, z + 0.005], [float(ndc_of(r + 2.25, H)), xs, z + 0.005],
                                   [float(ndc_of(r - 2.75, H)), xs, z + 0.005]], np.float32))
    return _scene("box_on_boundaries[H=%d]" % H, [faces], H, SIL_BLUR)


def giant(field=False):
    """One face with vertices at +-64 NDC over the whole image (more than 256 blocks: k_setup's `big` path), alone or
    behind 200 small faces."""
    H = 64
    faces = [_giant_face()]
    if field:
        f = _field_faces(H, 200, 11)
        faces = f[:77] + faces + f[77:]
    return _scene("giant" + ("+field" if field else ""), [faces], H, SIL_BLUR, giant_ids=[77 if field else 0])


def _far_faces(far):
    """Four faces over the whole image, one vertex each at +y, -y, +x and -x `far`: each of the four float -> int
    conversions of the face box (k_setup, the atlas gradient) leaves the range of an int in turn."""
    return [_giant_face(far), np.array([[-64.0, 64.0, 3.25], [0.0, -far, 3.25], [64.0, 64.0, 3.25]], np.float32),
            np.array([[-64.0, -64.0, 3.5], [-64.0, 64.0, 3.5], [far, 0.0, 3.5]], np.float32),
            np.array([[64.0, -64.0, 3.75], [-far, 0.0, 3.75], [64.0, 64.0, 3.75]], np.float32)]


def far_vertex(far, ways=False):
    """`giant` over the field with one vertex at y = `far`: 1e6 is in range of an int pixel index at H = 64, 4e9 is
    not (|NDC| H / 2 > 2^31: the conversion saturates).  ways: all four faces of _far_faces."""
    g = _far_faces(far)[:4 if ways else 1]
    f = _field_faces(64, 200, 11)
    return _scene("far_vertex[%g%s]" % (far, ",4 ways" if ways else ""), [f[:77] + g + f[77:]], 64, SIL_BLUR,
                  giant_ids=list(range(77, 77 + len(g))))


def far_vertex_batch(far):
    """The four faces of _far_faces as the backdrops of four meshes (each the nearest face at most pixels of its mesh:
    what the K = 1 walks and the atlas gradient see), behind 20 small faces each."""
    meshes = [_field_faces(64, 20, 20 + i) + [g] for i, g in enumerate(_far_faces(far))]
    return _scene("far_vertex_batch[%g]" % far, meshes, 64, 0.0, giant_ids=[20] * 4)


# ------------------------------------------------------------------------------------------------ definition
def _edge(px, py, ax, ay, bx, by):
    t1, t2 = (px - ax) * (by - ay), (py - ay) * (bx - ax)
    return t1 - t2, np.abs(t1) + np.abs(t2)


def _pld(px, py, ax, ay, bx, by, keps):
    bax, bay = bx - ax, by - ay
    l2 = bax * bax + bay * bay
    with np.errstate(all="ignore"):
        t = (bax * (px - ax) + bay * (py - ay)) / l2
        t = np.minimum(np.maximum(t, 0), 1)
        qx, qy = ax + t * bax, ay + t * bay
        d = (qx - px) * (qx - px) + (qy - py) * (qy - py)
    de = (px - bx) * (px - bx) + (py - by) * (py - by)
    return np.where(l2 <= keps, de, d), l2


def _eval(fv, H, blur, clip, dt):
    """oracle_rasterize's quantities for ONE mesh fv [F,3,3], operation for operation, in dtype dt -> arrays [H,H,F]."""
    fv = np.asarray(fv, np.float32).astype(dt)
    c = ndc_of(np.arange(H), H).astype(dt)
    yf, xf = c[:, None, None], c[None, :, None]
    (x0, y0, z0), (x1, y1, z1), (x2, y2, z2) = ((fv[:, i, 0], fv[:, i, 1], fv[:, i, 2]) for i in range(3))
    keps, blur_t = dt(K_EPS), dt(np.float32(blur))
    margin = dt(np.sqrt(np.float32(blur)))
    q = {}
    q["area"], q["s_area"] = _edge(x2, y2, x0, y0, x1, y1)
    q["nondeg"] = ~((q["area"] <= keps) & (q["area"] >= -keps))
    q["box"] = (np.minimum(np.minimum(x0, x1), x2) - margin, np.maximum(np.maximum(x0, x1), x2) + margin,
                np.minimum(np.minimum(y0, y1), y2) - margin, np.maximum(np.maximum(y0, y1), y2) + margin)
    bx0, bx1, by0, by1 = q["box"]
    q["inbox"] = ~((xf > bx1) | (xf < bx0) | (yf > by1) | (yf < by0))
    denom = q["area"] + keps
    q["denom"] = denom
    e = [_edge(xf, yf, x1, y1, x2, y2), _edge(xf, yf, x2, y2, x0, y0), _edge(xf, yf, x0, y0, x1, y1)]
    q["e"], q["s_e"] = [a for a, _ in e], [b for _, b in e]
    with np.errstate(all="ignore"):
        w = [a / denom for a in q["e"]]
        q["inside"] = (w[0] > 0) & (w[1] > 0) & (w[2] > 0)
        cc = w
        q["unclamped"] = np.ones(w[0].shape, bool)
        if clip:
            cc = [np.maximum(np.minimum(a, 1), 0) for a in w]
            q["unclamped"] = (cc[0] == w[0]) & (cc[1] == w[1]) & (cc[2] == w[2])
            s = np.maximum(cc[0] + cc[1] + cc[2], dt(np.float32(1e-5)))
            cc = [a / s for a in cc]
        q["pz"] = cc[0] * z0 + cc[1] * z1 + cc[2] * z2
        q["pz_num"] = q["e"][0] * z0 + q["e"][1] * z1 + q["e"][2] * z2          # pz * denom where nothing is clamped
        q["s_pz"] = sum(np.abs(z) * (np.abs(a) + s_ / np.abs(denom)) for z, a, s_ in zip((z0, z1, z2), cc, q["s_e"]))
    d01, l01 = _pld(xf, yf, x0, y0, x1, y1, keps)
    d02, l02 = _pld(xf, yf, x0, y0, x2, y2, keps)
    d12, l12 = _pld(xf, yf, x1, y1, x2, y2, keps)
    q["d"] = np.minimum(np.minimum(d01, d02), d12)
    q["l2"] = (l01, l02, l12)
    q["blur"] = blur_t
    return q


def _decide(q, exact_pz):
    """-> accepted [H,H,F], depth [H,H,F].  exact_pz (the float64 side): where no barycentric is clamped the sign of pz
    is that of (sum e_i z_i) / denom, whose numerator is exact for dyadic inputs -- a pz of exactly 0 stays 0, while the
    three rounded quotients e_i / (area + kEps) would leave +-1e-17 there."""
    pz = q["pz"]
    if exact_pz:
        pz = np.where(q["unclamped"] & (q["pz_num"] == 0), 0.0, pz)
    with np.errstate(invalid="ignore"):
        ok = q["nondeg"] & q["inbox"] & ~(pz < 0) & (q["inside"] | (q["d"] < q["blur"]))
    return ok & np.isfinite(pz), pz


_CACHE = {}


def _cached(fv, H, blur, clip):
    key = (fv.tobytes(), H, float(blur), bool(clip))
    if key not in _CACHE:
        if len(_CACHE) > 8:
            _CACHE.clear()
        _CACHE[key] = (_eval(fv, H, blur, clip, np.float64), _eval(fv, H, blur, clip, np.float32))
    return _CACHE[key]


def _kept(ok, pz, K):
    """The K nearest accepted faces of every pixel, ties to the lower id -> kept [H,H,F], and per pixel the depths
    either side of the cut (nan where nothing is cut)."""
    F = ok.shape[-1]
    key = np.where(ok, pz, np.inf)
    order = np.argsort(key, axis=-1, kind="stable")                   # stable: equal depths stay in id order
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.broadcast_to(np.arange(F), order.shape), -1)
    srt = np.take_along_axis(key, order, -1)
    cut = np.full(ok.shape[:2] + (2,), np.nan)
    if F > K:
        has = np.isfinite(srt[..., K])
        cut[has] = srt[..., K - 1:K + 1][has]
    return ok & (rank < K), cut, order


def definition(face_verts, H, K, blur, clip, N=1):
    """float64 restatement of oracle_rasterize's accept / reject rules for face_verts [N*F,3,3] -> dict:
    accepted [N,H,H,F] (every face that passes), depth [N,H,H,F], kept [N,H,H,F] (the K nearest, ties to the lower
    id), cut [N,H,H,2] (the depths either side of the truncation)."""
    fv = np.asarray(face_verts, np.float32).reshape(N, -1, 3, 3)
    out = dict(accepted=[], depth=[], kept=[], cut=[])
    for n in range(N):
        q64, _ = _cached(fv[n], H, blur, clip)
        ok, pz = _decide(q64, True)
        kept, cut, _ = _kept(ok, pz, K)
        for k, v in zip(("accepted", "depth", "kept", "cut"), (ok, pz, kept, cut)):
            out[k].append(v)
    return {k: np.stack(v) for k, v in out.items()}


REL, ABS_D = 1e-5, 1e-9


def margins(face_verts, H, K, blur, clip, N=1):
    """The distance of every decision quantity from its threshold, float64 side -> dict name -> (smallest margin that
    is not exactly 0, number of quantities exactly at the threshold, number of those that are NOT there in float32).
    Relative margins: |q - threshold| / max(|threshold|, sum of the magnitudes of q's terms).  Quantities:
      area   |area| against kEps, every face          l2    the three squared edge lengths against kEps
      w      the three edge functions against 0 and   pz    against 0: at every pixel inside the box of a face
      d      min distance against blur (absolute), where the pixel is not inside and blur > 0
      box    pixel centre against the four box sides, at the pixels every other rule accepts (elsewhere the box
             decides nothing: a pixel that fails it is further than sqrt(blur) from the face)
      cut    the depths either side of the truncation to K, relative to the magnitude of pz's terms"""
    fv = np.asarray(face_verts, np.float32).reshape(N, -1, 3, 3)
    res = {}

    def add(name, m, at32):
        """m: margins (0 = exactly at the threshold); at32: the same quantity is at its threshold in float32 as well."""
        m = np.asarray(m, np.float64).ravel()
        at32 = np.broadcast_to(at32, np.shape(m) if np.ndim(at32) == 0 else np.shape(at32)).ravel()
        zero = m == 0
        lo, n0, bad = res.get(name, (np.inf, 0, 0))
        if (~zero).any():
            lo = min(lo, float(m[~zero].min()))
        res[name] = (lo, n0 + int(zero.sum()), bad + int((zero & ~at32).sum()))

    for n in range(N):
        q, q32 = _cached(fv[n], H, blur, clip)
        nd = q["nondeg"]
        live = nd & q["inbox"]
        keps = float(K_EPS)
        # (an area that float32 evaluates EXACTLY -- collinear or repeated dyadic vertices: 0 -- is decided alike too)
        m_area = np.abs(np.abs(q["area"]) - keps) / np.maximum(q["s_area"], keps)
        same = q32["area"].astype(np.float64) == q["area"]
        add("area", np.where((m_area <= REL) & same, 0.0, m_area), (np.abs(q32["area"]) == K_EPS) | same)
        for l, l32 in zip(q["l2"], q32["l2"]):
            add("l2", (np.abs(l - keps) / np.maximum(l, keps))[nd], (l32 == K_EPS)[nd])
        for e, s, e32 in zip(q["e"], q["s_e"], q32["e"]):
            with np.errstate(invalid="ignore", divide="ignore"):
                add("w", np.where(e == 0, 0.0, np.abs(e) / s)[live], (e32 == 0)[live])
        ok, pz = _decide(q, True)
        with np.errstate(invalid="ignore", divide="ignore"):
            add("pz", np.where(pz == 0, 0.0, np.abs(pz) / q["s_pz"])[live], (q32["pz"] == 0)[live])
        if blur > 0:
            sel = live & ~q["inside"] & ~(pz < 0)
            add("d", np.abs(q["d"] - q["blur"])[sel], False)
        with np.errstate(invalid="ignore"):
            rest = nd & ~(pz < 0) & (q["inside"] | (q["d"] < q["blur"]))
        c = ndc_of(np.arange(H), H).astype(np.float64)
        c32 = ndc_of(np.arange(H), H)
        for side, side32, ax in zip(q["box"], q32["box"], (1, 1, 0, 0)):
            p = np.broadcast_to(c[None, :, None] if ax else c[:, None, None], rest.shape)
            p32 = np.broadcast_to(c32[None, :, None] if ax else c32[:, None, None], rest.shape)
            s64, s32 = np.broadcast_to(side, rest.shape), np.broadcast_to(side32, rest.shape)
            add("box", (np.abs(p - s64) / np.maximum(np.abs(p), np.abs(s64)))[rest], (p32 == s32)[rest])
        _, cut, order = _kept(ok, pz, K)
        has = np.isfinite(cut[..., 0])
        if has.any():
            a, b = order[..., K - 1][has], order[..., K][has]
            sp = np.maximum(np.take_along_axis(q["s_pz"], order[..., K - 1:K], -1)[..., 0][has],
                            np.take_along_axis(q["s_pz"], order[..., K:K + 1], -1)[..., 0][has])
            z32 = q32["pz"][has]
            same32 = z32[np.arange(len(a)), a] == z32[np.arange(len(a)), b]
            add("cut", (cut[..., 1] - cut[..., 0])[has] / sp, same32)
    return res


def check_margins(m):
    """-> list of complaints (empty: float32 and float64 decide every pixel alike)."""
    bad = []
    for name, (lo, n0, n_bad) in m.items():
        bar = ABS_D if name == "d" else REL
        if lo <= bar:
            bad.append("%s: smallest margin %.3g is within %.0e of its threshold" % (name, lo, bar))
        if n_bad:
            bad.append("%s: %d of %d quantities at the threshold in float64 are not there in float32" % (name, n_bad, n0))
    return bad


def cpu_scenes():
    """(scene, Ks) for the float64 comparison: everything but far_vertex[4e9] and the 1-ulp stacks."""
    out = [(shared_edge(), (1, 2, 4, 8)), (z_cross(), (1, 2, 4)), (area_eps(), (1, 2, 4, 8)), (short_edge(), (1, 2, 4)),
           (all_degenerate_mesh(8), (1, 4, 8, 10)), (all_degenerate_mesh(5), (1, 4, 10)),
           (box_on_boundaries(64), (1, 4, 8)), (box_on_boundaries(40), (1, 4, 8)), (giant(), (1, 4)),
           (giant(field=True), (1, 4, 8, 10)), (far_vertex(1e6), (1, 4, 10)), (far_vertex(1e6, ways=True), (1, 4, 10))]
    for K in (1, 2, 4, 8, 10, 20, 32):
        out += [(dup_stack(K, M), (K,)) for M in dup_stack_cases(K)]
    return out
