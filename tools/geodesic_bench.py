"""Timing of the geodesic handle distances (mesh_net.py:69-85, 523-544) at the reference's size: all pairs of a
642-vertex template at steiner = 15 (29,442 nodes, 1.18 M arcs, 117,784 bytes of LDS per workgroup, 642 workgroups).
ops.geodesic_distances (csrc/acfm_geodesic.hip, float32) against the host path of handles.py -- scipy's Dijkstra on the
same graph in float64 --, which is timed on a subset of the sources (its cost is per source) and scaled.  Events around
every iteration, warm-up, median.
--subdiv K: K SubdivideMeshes passes of the template first (1: 2562 vertices / 5120 faces / 7680 edges, which fits LDS
only up to steiner = 4).  --memory lds | device | auto: where the kernel keeps the node distances; with "device" the
LDS kernel is timed in the same run wherever the graph fits it, and the two matrices are compared bit for bit.
usage: python tools/geodesic_bench.py [--mesh horse] [--subdiv 0] [--steiner 15] [--memory lds] [--reps 20]
       [--host-sources 16] [--dump D.npy]
(--dump keeps the GPU's matrix, to compare two builds of the library bit for bit: ACFM_LIB selects the build)"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
from acfm_video_3d_reconstruction_amd import _lib, handles, ops

ap = argparse.ArgumentParser()
ap.add_argument("--mesh", default="horse")
ap.add_argument("--subdiv", type=int, default=0, help="SubdivideMeshes passes of the template")
ap.add_argument("--steiner", type=int, default=15)
ap.add_argument("--memory", default="lds", choices=ops.GEODESIC_MEMORY)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--host-sources", type=int, default=16, help="sources timed on the host path (0 = all)")
ap.add_argument("--dump", default=None, help="save the GPU's [V,V] matrix here (.npy)")
a = ap.parse_args()
d = torch.device("cuda:0")
m = np.load(os.path.join(ROOT, "tests", "golden", "meshes.npz"))
v, f = m[a.mesh + "_v"].astype(np.float32), m[a.mesh + "_f"]
if a.subdiv > 0:
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.ops import SubdivideMeshes
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.structures import Meshes
    sub = Meshes(verts=[torch.tensor(v)], faces=[torch.tensor(f)])
    for _ in range(a.subdiv):
        sub = SubdivideMeshes()(sub)
    v, f = sub.verts_packed().numpy().astype(np.float32), sub.faces_packed().numpy().astype(np.int64)
V = v.shape[0]
tv, tf = torch.tensor(v, device=d), torch.tensor(f, device=d)
E = handles.edge_tables(f, V)[0].shape[0]
lds_bytes = 16 + 4 * (V + a.steiner * E)
fits = lds_bytes <= ops.GEODESIC_LDS_MAX


def timed(memory):
    """-> (the matrix, the sorted times of a.reps calls in ms)."""
    D = ops.geodesic_distances(tv, tf, a.steiner, memory=memory)          # builds the tables
    for _ in range(a.warmup):
        ops.geodesic_distances(tv, tf, a.steiner, memory=memory)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)]
    for e0, e1 in ev:
        e0.record(); ops.geodesic_distances(tv, tf, a.steiner, memory=memory); e1.record()
    torch.cuda.synchronize()
    return D, sorted(e0.elapsed_time(e1) for e0, e1 in ev)


D, ms = timed(a.memory)
if a.dump:
    np.save(a.dump, D.cpu().numpy())
gpu_ms = ms[a.reps // 2]

k = V if a.host_sources <= 0 else min(a.host_sources, V)
src = np.linspace(0, V - 1, k).astype(np.int64)
t0 = time.perf_counter()
pos, r, c, w = handles.steiner_graph(v.astype(np.float64), f, a.steiner)
t_graph = time.perf_counter() - t0
t0 = time.perf_counter()
Dh = handles.geodesic_distance_matrix(v.astype(np.float64), f, a.steiner, src)
t_host = time.perf_counter() - t0 - t_graph            # (the call builds the graph once more)
err = float(np.abs(D[torch.as_tensor(src, device=d)].cpu().numpy() - Dh).max())
print("%s: V = %d, steiner = %d: %d nodes, %d arcs" % (a.mesh, V, a.steiner, pos.shape[0], r.shape[0]))
print("max |gpu - host| over %d sources: %.3e = %.3e of max D = %.4f" % (k, err, err / Dh.max(), Dh.max()))
print("LDS per workgroup: %d bytes (%s %d)" % (lds_bytes, "fits" if fits else "does not fit", ops.GEODESIC_LDS_MAX))
on_device = a.memory == "device" or (a.memory == "auto" and not fits)
print("GPU (memory = %s -> %s), all %d sources: median %.2f ms (min %.2f, max %.2f) of %d"
      % (a.memory, "device" if on_device else "lds", V, gpu_ms, ms[0], ms[-1], a.reps))
if on_device:
    ws = int(_lib.lib().acfm_geodesic_workspace_bytes(1, V, E, a.steiner, V, 0))
    G = ops.geodesic_device_workgroups(V)
    print("workspace: %d workgroups x %d bytes = %d bytes" % (G, ws // G, ws))
if a.memory == "device" and fits:
    D_lds, ms_lds = timed("lds")
    lds_ms = ms_lds[a.reps // 2]
    print("GPU (memory = lds) in the same run: median %.2f ms (min %.2f, max %.2f) of %d; device / lds = %.2f x; "
          "bit-equal: %s" % (lds_ms, ms_lds[0], ms_lds[-1], a.reps, gpu_ms / lds_ms, bool(torch.equal(D, D_lds))))
print("host: graph %.2f s; Dijkstra %.3f s per source over %d sources -> extrapolated %.1f s for all %d (%.0f x the GPU)"
      % (t_graph, max(t_host, 0.0) / k, k, max(t_host, 0.0) / k * V, V, max(t_host, 0.0) / k * V / (gpu_ms * 1e-3)))
