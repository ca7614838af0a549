"""The surface samples of the template fit (utils/geometry.py:110-111, `sample_points_from_meshes(mesh, 5000)` twice per
iteration), drawn on the GPU.

    sampler = SurfaceSampler(seed=0)
    points = pytorch3d_shim.ops.sample_points_from_meshes(meshes, 5000, sampler=sampler)

The reference draws with torch's global generator (one multinomial per mesh, two rand calls); here the draw is a
kernel (ops.sample_surface on acfm_sample.hip) whose only state is an int64 pair (seed, draw) in device memory,
advanced in stream order, exactly as boundary_sampling.BoundarySampler's.  An iteration of the fit can therefore be
captured into a hipGraph that draws afresh at every replay, and a test can say which points a draw must return.

The draws follow the reference's DISTRIBUTION -- faces with replacement in proportion to their area, then a uniform
point of each -- not its random stream.  One difference of substance: the areas are quantised to 24 bits of the mesh's
largest face (below), so a face smaller than 2^-24 of the largest face of its mesh is NEVER drawn, and the
probability of every other face is that of its area to within 2^-24 of the largest one's.

surface_sample_host is the definition in numpy; the kernel equals it bit for bit (tests/test_gpu_surface_sampler.py),
and it is what host tensors run when a sampler is given."""
import numpy as np

from .boundary_sampling import DrawState, philox4x32_10

_MASK32 = 0xFFFFFFFF
WEIGHT_BITS = 24


def face_norms_host(verts, faces):
    """Twice the area of every face in float32: n = sqrt((cx cx + cy cy) + cz cz) of (b - a) x (c - a), every
    operation rounded, in this order; 0 where the result is not finite or the face names a vertex outside [0, P)."""
    verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    faces = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    ok = ((faces >= 0) & (faces < verts.shape[0])).all(1)
    f = np.where(ok[:, None], faces, 0)
    a, b, c = verts[f[:, 0]], verts[f[:, 1]], verts[f[:, 2]]
    with np.errstate(all="ignore"):
        u, v = b - a, c - a
        cx = u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1]
        cy = u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2]
        cz = u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
        n = np.sqrt((cx * cx + cy * cy) + cz * cz)
    assert n.dtype == np.float32
    return np.where(ok & np.isfinite(n), n, np.float32(0)).astype(np.float32)


def face_weights_host(verts, faces):
    """The integer weights of ONE mesh's faces: q_f = floor((n_f / n_max) 2^24), the division in float32 (all zero when
    no face has an area).  A face below 2^-24 of the largest face has weight 0 and is never drawn."""
    n = face_norms_host(verts, faces)
    if n.size == 0 or not n.max() > 0:
        return np.zeros(n.shape, np.uint64)
    r = n / n.max()
    assert r.dtype == np.float32
    return np.floor(r * np.float32(1 << WEIGHT_BITS)).astype(np.uint64)


def surface_sample_host(seed, draw, verts, faces, first_idx, num_samples):
    """The definition of the draw.  verts [P,3], faces [F,3] packed, first_idx [N+1] (mesh m = faces
    [first_idx[m], first_idx[m+1])) -> (points [N,S,3] f32, face_idx [N,S] i32 rows of `faces`, uv [N,S,2] f32).
    Per mesh m: cdf = inclusive prefix sum (uint64) of face_weights_host; sample s takes (x0, x1, x2, x3) =
    Philox4x32-10 with key (seed lo, seed hi) and counter (s, m, draw lo, draw hi); target = ((x0 << 32 | x1) * total)
    >> 64 with total = cdf[-1]; the face is the first f with cdf_f > target (searchsorted side="right": faces of weight
    0 are skipped wherever they lie); u = (x2 >> 8) 2^-24, v = (x3 >> 8) 2^-24; su = sqrt(u), w = (1 - su, su (1 - v),
    su v), point = (w0 a + w1 b) + w2 c in float32.  A mesh without faces, or with total == 0: points 0, face -1, uv 0."""
    seed, draw = int(seed) & 0xFFFFFFFFFFFFFFFF, int(draw) & 0xFFFFFFFFFFFFFFFF
    verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    faces = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    first = [int(x) for x in np.asarray(first_idx).reshape(-1)]
    N, S, F = len(first) - 1, int(num_samples), faces.shape[0]
    if N < 1 or any(b < a for a, b in zip([0] + first, first)) or first[-1] > F:
        raise ValueError("surface_sample_host: first_idx must be non-decreasing within [0, F], got %s" % (first,))
    points = np.zeros((N, S, 3), np.float32)
    face_idx = np.full((N, S), -1, np.int32)
    uv = np.zeros((N, S, 2), np.float32)
    s = np.arange(S, dtype=np.uint64)
    for m in range(N):
        f0, f1 = first[m], first[m + 1]
        cdf = np.cumsum(face_weights_host(verts, faces[f0:f1]), dtype=np.uint64)
        total = int(cdf[-1]) if cdf.size else 0
        if total == 0:
            continue
        x = philox4x32_10((s, m, draw & _MASK32, draw >> 32), (seed & _MASK32, seed >> 32))
        r = [(int(a) << 32) | int(b) for a, b in zip(x[0], x[1])]
        target = np.array([(v * total) >> 64 for v in r], dtype=np.uint64)          # exact: Python integers
        f = np.searchsorted(cdf, target, side="right").astype(np.int64) + f0
        u = (x[2] >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
        v = (x[3] >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
        su = np.sqrt(u)
        w0, w1, w2 = np.float32(1) - su, su * (np.float32(1) - v), su * v
        a, b, c = verts[faces[f, 0]], verts[faces[f, 1]], verts[faces[f, 2]]
        points[m] = (w0[:, None] * a + w1[:, None] * b) + w2[:, None] * c
        face_idx[m] = f.astype(np.int32)
        uv[m, :, 0], uv[m, :, 1] = u, v
    return points, face_idx, uv


class SurfaceSampler(DrawState):
    """Holds the state (seed, draw) of the surface draw: one int64 [2] tensor per device, created on first use there
    (before capturing a graph call state_on(device), or sample once eagerly), and a draw counter of its own for host
    tensors."""

    def __init__(self, seed=0):
        super().__init__(seed)
        self.host_draw = 0

    def reseed(self, seed, draw=0):
        """Restart every sequence -- each device's and the host's -- at (seed, draw)."""
        super().reseed(seed, draw)
        self.host_draw = int(draw)
        return self

    def draw_host(self, verts, faces, first_idx, num_samples):
        """surface_sample_host at the host sequence's (seed, draw); advances that counter."""
        out = surface_sample_host(self.seed, self.host_draw, verts, faces, first_idx, num_samples)
        self.host_draw += 1
        return out
