"""Geodesic handles (csrc/acfm_geodesic.hip)."""
import torch

from .. import _lib


GEODESIC_MAX_STEINER = 20        # ACFM_GEODESIC_MAX_STEINER: 3 m + 3 boundary nodes of a face fit one wave
GEODESIC_LDS_MAX = 153600        # ACFM_GEODESIC_LDS_MAX


def geodesic_max_steiner(V, E):
    """The largest steiner count whose graph (V + m E nodes, 4 bytes each) fits one workgroup's LDS; -1 if none does."""
    fits = [m for m in range(GEODESIC_MAX_STEINER + 1)
            if 0 < int(_lib.lib().acfm_geodesic_lds_bytes(int(V), int(E), m)) <= GEODESIC_LDS_MAX]
    return max(fits) if fits else -1


GEODESIC_MEMORY = ("lds", "device", "auto")


def geodesic_memory(memory):
    """`memory` of geodesic_distances, validated: one of "lds", "device", "auto"."""
    if memory not in GEODESIC_MEMORY:
        raise ValueError('memory must be one of "lds", "device", "auto", got %r' % (memory,))
    return memory


def geodesic_device_workgroups(items, max_workgroups=None):
    """The grid of the device-memory kernel for `items` = S N (source, mesh) pairs: min(items, max_workgroups),
    max_workgroups None = two per CU of the current device."""
    one = int(_lib.lib().acfm_geodesic_workspace_bytes(1, 1, 0, 0, 1, 1))
    return int(_lib.lib().acfm_geodesic_workspace_bytes(1, 1, 0, 0, int(items), int(max_workgroups or 0))) // one


def geodesic_distances(verts, faces, steiner=15, sources=None, memory="lds", max_workgroups=None):
    """Surface distances between the vertices of a mesh, for the handle weights of mesh_net.py:69-85, 523-544 (there
    gdist.local_gdist_matrix): shortest paths on the edge-Steiner graph -- `steiner` = m points on every edge, inside
    every face all pairs of its 3 + 3 m boundary nodes joined by their Euclidean distance.  An upper bound of the exact
    geodesic (DESIGN.md "Geodesic handles": under 0.2 % at the default m = 15), +inf between components, 0 on the
    diagonal; the same bits on every run.
    verts [V,3] or [N,V,3] float32 on the GPU, faces [F,3] (one topology for all N), sources: None (all V vertices) or
    S vertex ids (a sequence or an integer tensor; any order, repeats allowed) -> [S,V] or [N,S,V] float32, detached (the
    reference computes these in numpy).
    memory = "lds": one launch, one workgroup per (source, mesh), the graph in LDS: a graph of more than 153,584 / 4
    nodes is refused with the largest steiner count that fits.  "device": the same relaxation with the distances in a
    per-call workspace (one row of V + m E floats per resident workgroup), any graph, the same bits; a persistent grid
    of min(S N, max_workgroups) workgroups, max_workgroups None = two per CU.  "auto": "lds" where the graph fits,
    else "device".
    The int32 edge tables are built once per faces tensor (Meshes.geodesic_tables_packed) and `sources` is uploaded per
    call: inside a graph capture the op runs only when the tables exist and `sources` is None or an int32 tensor on the
    device, and it raises otherwise."""
    from ..pytorch3d_shim.structures import Meshes   # (the shim is built on ops: it cannot be imported at load time)
    if not (torch.is_tensor(verts) and torch.is_tensor(faces)):
        raise ValueError("geodesic_distances: verts and faces must be tensors (handles.geodesic_distance_matrix takes arrays)")
    _lib.require_gpu(verts, faces)
    if verts.dim() not in (2, 3) or verts.shape[-1] != 3 or verts.shape[-2] < 1 or verts.shape[0] < 1:
        raise ValueError("geodesic_distances: verts [V,3] or [N,V,3] expected, got %s" % (tuple(verts.shape),))
    if verts.dtype != torch.float32:
        raise ValueError("geodesic_distances: verts must be float32, got %s" % verts.dtype)
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] < 1 or faces.dtype.is_floating_point:
        raise ValueError("geodesic_distances: faces [F,3] of integers expected (one topology), got %s %s"
                         % (faces.dtype, tuple(faces.shape)))
    if faces.device != verts.device:
        raise ValueError("geodesic_distances: verts are on %s, faces on %s" % (verts.device, faces.device))
    m = int(steiner)
    if m != steiner or not 0 <= m <= GEODESIC_MAX_STEINER:
        raise ValueError("steiner must be an integer in [0, %d] (3 steiner + 3 nodes per face, one wave), got %r"
                         % (GEODESIC_MAX_STEINER, steiner))
    geodesic_memory(memory)
    if max_workgroups is not None and (int(max_workgroups) != max_workgroups or int(max_workgroups) < 1):
        raise ValueError("max_workgroups must be None or a positive integer, got %r" % (max_workgroups,))
    dev = verts.device
    v = verts.detach().contiguous()
    batched = v.dim() == 3
    v3 = v if batched else v[None]
    N, V = v3.shape[0], v3.shape[1]
    capturing = torch.cuda.is_current_stream_capturing()
    mesh = Meshes(verts=[v3[0]], faces=[faces])
    if not mesh.has_geodesic_tables():
        if capturing:
            raise RuntimeError("geodesic_distances cannot build its edge tables inside a graph capture: call it once on "
                               "this faces tensor before capturing")
        lo, hi = int(faces.min()), int(faces.max())
        if lo < 0 or hi >= V:
            raise ValueError("faces hold vertex ids in [%d, %d], the mesh has %d vertices" % (lo, hi, V))
    f32, e32, fe32 = mesh.geodesic_tables_packed()
    F_, E = f32.shape[0], e32.shape[0]
    with torch.cuda.device(dev):
        need = int(_lib.lib().acfm_geodesic_lds_bytes(V, E, m))
    fits = 0 < need <= GEODESIC_LDS_MAX
    if memory == "lds" and not fits:
        raise ValueError("geodesic_distances: %d vertices + %d x %d edge points need %d bytes of LDS, a workgroup has %d; "
                         "the largest steiner that fits this mesh is %d" % (V, m, E, 16 + 4 * (V + m * E),
                                                                           GEODESIC_LDS_MAX, geodesic_max_steiner(V, E)))
    src = None
    if sources is not None:
        if torch.is_tensor(sources) and sources.is_cuda and sources.dtype == torch.int32:
            src = sources.detach().contiguous()
        elif capturing:
            raise RuntimeError("geodesic_distances inside a graph capture: sources must be None or an int32 tensor on "
                               "the device (anything else is uploaded)")
        else:
            src = torch.as_tensor(sources).detach().to(device=dev, dtype=torch.int32).contiguous()
        if src.dim() != 1 or src.numel() < 1 or src.device != dev:
            raise ValueError("sources: S >= 1 vertex ids on %s expected, got %s on %s" % (dev, tuple(src.shape), src.device))
        if not capturing:
            lo, hi = int(src.min()), int(src.max())
            if lo < 0 or hi >= V:
                raise ValueError("sources hold vertex ids in [%d, %d], the mesh has %d vertices" % (lo, hi, V))
    S = V if src is None else src.shape[0]
    out = torch.empty((N, S, V), dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    if memory == "lds" or (memory == "auto" and fits):
        _lib.call("acfm_geodesic_distances", dev, v3, f32, e32, fe32, N, V, F_, E, m, src, S, out, status)
    else:
        cap = int(max_workgroups or 0)
        with torch.cuda.device(dev):
            ws_bytes = int(_lib.lib().acfm_geodesic_workspace_bytes(N, V, E, m, S, cap))
        if ws_bytes == 0:
            raise ValueError("geodesic_distances: no workspace size for N = %d, V = %d, E = %d, steiner = %d, S = %d"
                             % (N, V, E, m, S))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        _lib.call("acfm_geodesic_distances_dev", dev, v3, f32, e32, fe32, N, V, F_, E, m, src, S, out, status, cap, ws,
                  ws_bytes)
    if not capturing:       # (a captured call cannot read it: a workgroup that gave up leaves a row of NaN)
        st = int(status.item())
        if st:
            raise RuntimeError("acfm_geodesic_distances: %s" % {
                1: "no fixed point after V + m E sweeps",
                2: "a source outside [0, V)"}.get(st, "status %d" % st))
    return out if batched else out[0]
