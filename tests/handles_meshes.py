"""Meshes with a known geodesic, shared by test_handles.py and test_gpu_handles.py (not a test module).
Every builder returns (verts [V,3] float64, faces [F,3] int64); exact_* return the analytic [V,V] geodesic."""
import numpy as np


def _cells(keep, n=4):
    """Unit cells (i, j) of an n x n grid with keep(i, j), two triangles each, the diagonal alternating with
    (i + j) % 2; only vertices of kept cells are numbered."""
    ids, verts, faces = {}, [], []

    def vid(i, j):
        if (i, j) not in ids:
            ids[(i, j)] = len(verts)
            verts.append((float(i), float(j), 0.0))
        return ids[(i, j)]

    for i in range(n):
        for j in range(n):
            if not keep(i, j):
                continue
            a, b, c, d = vid(i, j), vid(i + 1, j), vid(i + 1, j + 1), vid(i, j + 1)
            faces += [(a, b, c), (a, c, d)] if (i + j) % 2 == 0 else [(a, b, d), (b, c, d)]
    return np.asarray(verts, np.float64), np.asarray(faces, np.int64)


def square():
    return _cells(lambda i, j: True)


def l_shape():
    return _cells(lambda i, j: not (i >= 2 and j >= 2))


def _euclid(v):
    return np.linalg.norm(v[:, None] - v[None], axis=-1)


def exact_square(v):
    return _euclid(v)


def exact_l_shape(v):
    """Euclidean where the segment stays inside the L, otherwise through the reflex corner (2, 2)."""
    D = _euclid(v)
    corner = np.array([2.0, 2.0, 0.0])
    dc = np.linalg.norm(v - corner, axis=1)
    for a in range(v.shape[0]):
        for b in range(v.shape[0]):
            p, q = v[a], v[b]
            if p[0] > 2 and q[1] > 2:          # p in the arm x > 2 (so y <= 2), q in the arm y > 2 (so x <= 2)
                y_at_2 = q[1] + (2 - q[0]) / (p[0] - q[0]) * (p[1] - q[1])
                if y_at_2 > 2:                 # the segment passes over the removed cells
                    D[a, b] = D[b, a] = dc[a] + dc[b]
    return D


PRISM_SIDES, PRISM_RINGS, PRISM_DZ = 7, 4, 0.9


def prism():
    """Open 7-sided prism: radius 1, 4 rings 0.9 apart, two triangles per quad, no caps.  Vertex = ring * 7 + side."""
    ang = 2 * np.pi * np.arange(PRISM_SIDES) / PRISM_SIDES
    verts = np.array([(np.cos(t), np.sin(t), PRISM_DZ * r) for r in range(PRISM_RINGS) for t in ang], np.float64)
    faces = []
    for r in range(PRISM_RINGS - 1):
        for k in range(PRISM_SIDES):
            a, b = r * PRISM_SIDES + k, r * PRISM_SIDES + (k + 1) % PRISM_SIDES
            c, d = b + PRISM_SIDES, a + PRISM_SIDES
            faces += [(a, b, c), (a, c, d)]
    return verts, np.asarray(faces, np.int64)


def jittered_prism(seed=1):
    """The prism with every vertex moved by N(0, 0.05^2) per coordinate, rounded to float32: no symmetric ties left.
    (Seed 1 was picked when the tests were written: every farthest-point step up to 8 handles is decided by more than
    6e-3 of the largest distance; test_gpu_handles asserts the margin it needs.)"""
    v, f = prism()
    v = v + np.random.default_rng(seed).normal(scale=0.05, size=v.shape)
    return v.astype(np.float32).astype(np.float64), f


def exact_prism(v):
    """sqrt(dz^2 + min(ds, P - ds)^2): the sides unroll into a flat strip."""
    side = 2 * np.sin(np.pi / PRISM_SIDES)
    ring, k = np.divmod(np.arange(v.shape[0]), PRISM_SIDES)
    ds = side * np.abs(k[:, None] - k[None])
    ds = np.minimum(ds, PRISM_SIDES * side - ds)
    dz = PRISM_DZ * (ring[:, None] - ring[None])
    return np.sqrt(dz ** 2 + ds ** 2)


def u_strip():
    """A 1 x 9 strip of unit quads folded at its two middle creases into a staple: cells 0-3 one arm, cell 4 the base,
    cells 5-8 the other arm, the arms parallel and one unit apart.  Vertex = 2 * column + row; the tips are columns 0
    and 9."""
    verts, faces = [], []
    for c in range(10):
        x, z = (0.0, 4.0 - c) if c <= 4 else (1.0, c - 5.0)
        verts += [(x, 0.0, z), (x, 1.0, z)]
    for c in range(9):
        a, b, d, e = 2 * c, 2 * c + 1, 2 * c + 2, 2 * c + 3
        faces += [(a, d, e), (a, e, b)]
    return np.asarray(verts, np.float64), np.asarray(faces, np.int64)


def edge_graph_dijkstra(v, f):
    """Dijkstra on the mesh's edge graph, written out independently of the package (float64)."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import dijkstra
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0)
    e = np.unique(np.sort(e, 1), axis=0)
    w = np.linalg.norm(v[e[:, 0]] - v[e[:, 1]], axis=1)
    n = v.shape[0]
    return dijkstra(coo_matrix((w, (e[:, 0], e[:, 1])), shape=(n, n)).tocsr(), directed=False)


KNOWN = {"square": (square, exact_square), "L": (l_shape, exact_l_shape), "prism": (prism, exact_prism)}
