"""Lit shading (acfm_light.hip): vertex / face normals, the lighting function at points, and the
per-fragment Phong / flat shader.  Lights, materials and the camera centre are constants here (LightConstants): a
light or material that requires a gradient takes the shim's composition of torch operators instead."""
import collections

import torch

from .. import _lib
from .base import _f32c, _i64c
from .fragments import _det_ws, _frag_planes, _shade_storage

SHADE_MODES = ("phong", "flat")

IncidenceTable = collections.namedtuple("IncidenceTable", "offsets corners num_verts num_faces")
LightConstants = collections.namedtuple("LightConstants", "consts point num_meshes")


def incidence_table(faces_packed, num_verts):
    """The vertex-to-incident-corner table of packed faces [F,3], in CSR form: offsets [V+1] int32 and corners [3F]
    int32 = 3 f + i, the corners of vertex v at corners[offsets[v]:offsets[v+1]], ascending (so ascending by face).
    Every corner with a vertex id in [0, V) appears exactly once; the tail past offsets[V] is -1.  Topology only:
    built on the host (one read of the faces), once per faces tensor -- Meshes memoises it."""
    import numpy as np
    if faces_packed.dim() != 2 or faces_packed.shape[1] != 3 or faces_packed.shape[0] < 1:
        raise ValueError("faces_packed must be [F,3], got %s" % (tuple(faces_packed.shape),))
    V, F = int(num_verts), int(faces_packed.shape[0])
    if V < 1:
        raise ValueError("num_verts must be >= 1, got %d" % V)
    ids = faces_packed.detach().cpu().numpy().astype(np.int64).reshape(-1)
    valid = (ids >= 0) & (ids < V)
    order = np.argsort(ids, kind="stable")
    order = order[valid[order]]
    offsets = np.zeros(V + 1, np.int32)
    offsets[1:] = np.cumsum(np.bincount(ids[valid], minlength=V))
    corners = np.full(3 * F, -1, np.int32)
    corners[:order.size] = order
    dev = faces_packed.device
    return IncidenceTable(torch.from_numpy(offsets).to(dev), torch.from_numpy(corners).to(dev), V, F)


def _check_table(table, V, F, device):
    if not isinstance(table, IncidenceTable) or table.num_verts != V or table.num_faces != F:
        raise ValueError("table must be incidence_table(faces_packed, %d) of these %d faces, got %r"
                         % (V, F, (getattr(table, "num_verts", None), getattr(table, "num_faces", None))))
    _lib.require_gpu(table.offsets, table.corners)


def _check_f32(**tensors):
    for name, t in tensors.items():
        if t.dtype != torch.float32:
            raise ValueError("%s must be float32 (half storage is not supported on the shader path), got %s"
                             % (name, t.dtype))


class _VertexNormals(torch.autograd.Function):
    """acfm_vertex_normals{,_backward} -> (verts_normals [V,3], faces_normals [F,3]); gradient to verts."""

    @staticmethod
    def forward(ctx, verts, faces, table):
        v, f = _f32c(verts), _i64c(faces)
        V, F = v.shape[0], f.shape[0]
        vn = torch.empty((V, 3), dtype=torch.float32, device=v.device)
        fn = torch.empty((F, 3), dtype=torch.float32, device=v.device)
        _lib.call("acfm_vertex_normals", v.device, v, f, table.offsets, table.corners, V, F, vn, fn)
        ctx.save_for_backward(v, f)
        ctx.table = table
        ctx.set_materialize_grads(False)
        return vn, fn

    @staticmethod
    def backward(ctx, gvn, gfn):
        if not ctx.needs_input_grad[0] or (gvn is None and gfn is None):
            return None, None, None
        v, f = ctx.saved_tensors
        V, F = v.shape[0], f.shape[0]
        gvn, gfn = (_f32c(g) if g is not None else None for g in (gvn, gfn))
        gv = torch.empty_like(v)
        nb = 12 * V if gvn is not None else 0
        ws = torch.empty(nb, dtype=torch.uint8, device=v.device) if nb else None
        _lib.call("acfm_vertex_normals_backward", v.device, v, f, ctx.table.offsets, ctx.table.corners, gvn, gfn, V, F,
                  gv, ws, nb)
        return gv, None, None


def vertex_normals(verts_packed, faces_packed, table):
    """PyTorch3D 0.3.0 Meshes.verts_normals_packed / faces_normals_packed: verts_packed [V,3], faces_packed [F,3] int64,
    table = incidence_table(faces_packed, V) -> (verts_normals [V,3], faces_normals [F,3]).  A vertex normal is the sum
    of the unnormalised cross products taken at its own corner of every incident face, x / max(|x|, 1e-6); a face normal
    is normalize((v2 - v1) x (v0 - v1)).  Differentiable with respect to verts_packed; both directions are gathers per
    vertex (no atomics, any valence), bit-reproducible and capturable."""
    if verts_packed.dim() != 2 or verts_packed.shape[1] != 3 or verts_packed.shape[0] < 1:
        raise ValueError("verts_packed must be [V,3], got %s" % (tuple(verts_packed.shape),))
    if faces_packed.dim() != 2 or faces_packed.shape[1] != 3 or faces_packed.shape[0] < 1:
        raise ValueError("faces_packed must be [F,3], got %s" % (tuple(faces_packed.shape),))
    _check_f32(verts_packed=verts_packed)
    _lib.require_gpu(verts_packed, faces_packed)
    _check_table(table, verts_packed.shape[0], faces_packed.shape[0], verts_packed.device)
    return _VertexNormals.apply(verts_packed, faces_packed, table)


def light_constants(ambient, diffuse, specular, light_vector, camera_center, shininess, num_meshes, point):
    """The per-mesh constants of the lit kernels -> LightConstants(consts [N,16], point, N): ambient / diffuse /
    specular = light colour x material colour, light_vector = the direction (point=False) or location (point=True),
    camera_center, each [3], [1,3] or [N,3]; shininess a number or [1] / [N].  None of them may require a gradient."""
    N = int(num_meshes)
    cols = []
    for name, t in (("ambient", ambient), ("diffuse", diffuse), ("specular", specular), ("light_vector", light_vector),
                    ("camera_center", camera_center)):
        if t.requires_grad:
            raise ValueError("%s is a constant of the fused lighting path (no gradient); use the composition" % name)
        t = t.detach().to(torch.float32).reshape(-1, 3)
        if t.shape[0] not in (1, N):
            raise ValueError("%s must be [3], [1,3] or [N,3] with N = %d, got %s" % (name, N, tuple(t.shape)))
        cols.append(t.expand(N, 3))
    _lib.require_gpu(*cols)
    dev = cols[0].device
    if torch.is_tensor(shininess):
        if shininess.requires_grad:
            raise ValueError("shininess is a constant of the fused lighting path (no gradient); use the composition")
        s = shininess.detach().to(device=dev, dtype=torch.float32).reshape(-1, 1)
        if s.shape[0] not in (1, N):
            raise ValueError("shininess must be a number, [1] or [N] with N = %d, got %s" % (N, tuple(shininess.shape)))
        s = s.expand(N, 1)
    else:
        s = _lib.const([float(shininess)], dev).reshape(1, 1).expand(N, 1)
    return LightConstants(torch.cat(cols + [s], dim=1).contiguous(), int(bool(point)), N)


def _check_lights(lights, N):
    if not isinstance(lights, LightConstants) or lights.num_meshes != N or tuple(lights.consts.shape) != (N, 16):
        raise ValueError("lights must be light_constants(...) of %d meshes, got %r" % (N, type(lights).__name__))
    _lib.require_gpu(lights.consts)


class _LightPoints(torch.autograd.Function):
    """acfm_light_points{,_backward}; gradients to points, normals and colours."""

    @staticmethod
    def forward(ctx, points, normals, colours, mesh_idx, lights):
        p, n, c = _f32c(points), _f32c(normals), _f32c(colours)
        m = _i64c(mesh_idx) if mesh_idx is not None else None
        out = torch.empty_like(p)
        _lib.call("acfm_light_points", p.device, p, n, c, m, lights.consts, lights.point, p.shape[0],
                  lights.num_meshes, out)
        ctx.save_for_backward(p, n, c, m)
        ctx.lights = lights
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    def backward(ctx, g):
        need = ctx.needs_input_grad[:3]
        if g is None or not any(need):
            return (None,) * 5
        p, n, c, m = ctx.saved_tensors
        gp, gn, gc = (torch.empty_like(p) if k else None for k in need)
        _lib.call("acfm_light_points_backward", p.device, p, n, c, m, ctx.lights.consts, ctx.lights.point, _f32c(g),
                  p.shape[0], ctx.lights.num_meshes, gp, gn, gc)
        return gp, gn, gc, None, None


def light_points(points, normals, colours, lights, mesh_idx=None):
    """The lighting function of PyTorch3D 0.3.0's lights at M points (Gouraud's vertex stage): points, normals, colours
    [M,3] -> [M,3] = (ambient + diffuse relu(n.l)) colours + specular relu(v.r)^shininess [n.l > 0], with the constants
    lights = light_constants(...) of mesh mesh_idx[m] ([M] int64; None: one mesh).  Differentiable with respect to
    points, normals and colours."""
    for name, t in (("points", points), ("normals", normals), ("colours", colours)):
        if t.dim() != 2 or t.shape[1] != 3 or t.shape[0] < 1 or t.shape != points.shape:
            raise ValueError("%s must be [M,3] like points %s, got %s" % (name, tuple(points.shape), tuple(t.shape)))
    _check_f32(points=points, normals=normals, colours=colours)
    if mesh_idx is not None and tuple(mesh_idx.shape) != (points.shape[0],):
        raise ValueError("mesh_idx must be [M] = [%d], got %s" % (points.shape[0], tuple(mesh_idx.shape)))
    if not isinstance(lights, LightConstants):
        raise ValueError("lights must be light_constants(...), got %r" % type(lights).__name__)
    if mesh_idx is None and lights.num_meshes != 1:
        raise ValueError("mesh_idx is required with the constants of %d meshes" % lights.num_meshes)
    _lib.require_gpu(points, normals, colours, mesh_idx)
    _check_lights(lights, lights.num_meshes)
    return _LightPoints.apply(points, normals, colours, mesh_idx, lights)


class _PhongShade(torch.autograd.Function):
    """acfm_phong_shade{,_backward} + acfm_corner_gather -> colors [N,H,W,K,3]; gradients to bary_coords, texels, verts
    and normals (through the face-corner buffer and the incidence table: the last two leave without atomics)."""

    @staticmethod
    def forward(ctx, bary, texels, verts, normals, p2f, faces, lights, table, flat):
        p2f, b, t = _i64c(p2f), _f32c(bary), _f32c(texels)
        v, n, f = _f32c(verts), _f32c(normals), _i64c(faces)
        N, H, W, K = p2f.shape
        out = torch.empty(p2f.shape + (3,), dtype=torch.float32, device=p2f.device)
        tune = _lib.tuning()[1]
        dims = (N * H * W, K, H * W, f.shape[0], v.shape[0], N)
        _lib.call("acfm_phong_shade", p2f.device, p2f, b, t, v, f, n, lights.consts, lights.point, flat, *dims, out,
                  _lib.tuning_ptr(tune))
        ctx.save_for_backward(p2f, b, t, v, n, f)
        ctx.cfg = (dims, lights, table, flat, tune)
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    def backward(ctx, g):
        need_b, need_t, need_v, need_n = ctx.needs_input_grad[:4]
        if g is None or not (need_b or need_t or need_v or need_n):
            return (None,) * 9
        p2f, b, t, v, n, f = ctx.saved_tensors
        dims, lights, table, flat, tune = ctx.cfg
        gb = torch.empty_like(b) if need_b else None
        gt = torch.empty_like(t) if need_t else None
        corners = torch.empty((f.shape[0], 3, 6), dtype=torch.float32, device=v.device) if need_v or need_n else None
        ws, nb = _det_ws(tune, corners.numel(), v.device) if corners is not None else (None, 0)
        _lib.call("acfm_phong_shade_backward", p2f.device, p2f, b, t, v, f, n, lights.consts, lights.point, flat,
                  _f32c(g), *dims, gt, gb, corners, ws, nb, _lib.tuning_ptr(tune))
        gv = gn = None
        if corners is not None:
            gv, gn = torch.empty_like(v), torch.empty_like(n)
            _lib.call("acfm_corner_gather", v.device, corners, table.offsets, table.corners, v.shape[0], f.shape[0],
                      flat, gv, gn)
        return gb, gt, gv if need_v else None, gn if need_n else None, None, None, None, None, None


def phong_shade(fragments, verts, faces, normals, texels, lights, table, mode="phong", storage="f32"):
    """PyTorch3D 0.3.0 phong_shading (mode="phong") / flat_shading (mode="flat") over Fragments in one kernel: colors
    [N,H,W,K,3] = (ambient + diffuse) texels + specular at each slot's position and normal.  verts [V,3] and faces
    [F,3] int64 packed; normals = the vertex normals [V,3] (phong: position and normal are interpolated by the
    barycentrics inside the kernel) or the face normals [F,3] (flat: the face's mean position and its normal);
    lights = light_constants(...) of the N images' meshes; table = incidence_table(faces, V).  A slot without a face is
    shaded at position and normal 0.  Differentiable with respect to texels, verts, normals and fragments.bary_coords
    (the last only when it requires a gradient); _lib.raster_tuning(deterministic=True) makes the backward
    bit-reproducible."""
    _shade_storage(storage)
    if mode not in SHADE_MODES:
        raise ValueError("mode=%r is not supported (one of %s)" % (mode, SHADE_MODES))
    p2f, zbuf, bary, dists = _frag_planes(fragments)
    N = int(p2f.shape[0])
    if p2f.numel() == 0:
        raise ValueError("pix_to_face is empty: %s" % (tuple(p2f.shape),))
    if tuple(texels.shape) != tuple(p2f.shape) + (3,):
        raise ValueError("texels must be [N,H,W,K,3] = %s, got %s" % (tuple(p2f.shape) + (3,), tuple(texels.shape)))
    if verts.dim() != 2 or verts.shape[1] != 3 or verts.shape[0] < 1:
        raise ValueError("verts must be packed [V,3], got %s" % (tuple(verts.shape),))
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] < 1:
        raise ValueError("faces must be packed [F,3], got %s" % (tuple(faces.shape),))
    rows = faces.shape[0] if mode == "flat" else verts.shape[0]
    if tuple(normals.shape) != (rows, 3):
        raise ValueError("normals must be [%d,3] in mode %r, got %s" % (rows, mode, tuple(normals.shape)))
    _check_f32(bary_coords=bary, texels=texels, verts=verts, normals=normals)
    _lib.require_gpu(p2f, bary, texels, verts, faces, normals)
    _check_lights(lights, N)
    _check_table(table, verts.shape[0], faces.shape[0], verts.device)
    return _PhongShade.apply(bary, texels, verts, normals, p2f, faces, lights, table, SHADE_MODES.index(mode))
