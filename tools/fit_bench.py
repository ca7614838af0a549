"""Timing of one iteration of the template fit (utils/geometry.py:102-135): the 642-vertex level-3 sphere plus an offset
against a target mesh, 5000 + 5000 surface samples, chamfer + edge + normal consistency + uniform Laplacian, forward and
backward.  Two variants: the shim's operators (HIP kernels), and the same step composed from torch ops on the GPU
(torch.cdist + min, index ops) -- an independent formulation, not the code under test.  Events around every iteration,
warm-up, median.
--sampler draws the surface samples with surface_sampling.SurfaceSampler (the kernel of ops.sample_surface) instead of
torch.multinomial / torch.rand.  --loop N adds the whole loop, template_fit.fit_verts_to_mesh for N iterations, three
ways: eager with torch's draws, eager with the kernel's, and one captured iteration replayed (wall time, synchronised).
usage: python tools/fit_bench.py [--reps 100] [--samples 5000] [--sampler] [--loop 2000]"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
from acfm_video_3d_reconstruction_amd import pytorch3d_shim as p3d
from acfm_video_3d_reconstruction_amd.pytorch3d_shim.structures import Meshes
from acfm_video_3d_reconstruction_amd.surface_sampling import SurfaceSampler

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=100)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--samples", type=int, default=5000)
ap.add_argument("--sampler", action="store_true", help="draw with SurfaceSampler (the kernel) instead of torch's generator")
ap.add_argument("--loop", type=int, default=0, help="also time the whole fit loop for this many iterations, three ways")
a = ap.parse_args()
assert a.reps >= 50
d = torch.device("cuda:0")
torch.manual_seed(0)
sphere = p3d.utils.ico_sphere(3, d)
base, faces = sphere.verts_list()[0], sphere.faces_list()[0]
target = Meshes(verts=[base * torch.tensor([1.0, 0.6, 0.4], device=d)], faces=[faces])
offset = (0.01 * torch.randn_like(base)).requires_grad_(True)
S = a.samples
# the constant tables of the torch variant (topology only), built once as the shim builds its own
edges = sphere.edges_packed()
quads = sphere.normal_pairs_packed()[0]
deg = torch.zeros(base.shape[0], device=d).index_add_(0, edges.reshape(-1), torch.ones(2 * edges.shape[0], device=d))


SAMPLER = SurfaceSampler(seed=0) if a.sampler else None


def samples(mesh):
    return p3d.ops.sample_points_from_meshes(mesh, S, sampler=SAMPLER)


def hip_terms(mesh, xs, ys):
    return (lambda: p3d.loss.chamfer_distance(xs, ys)[0], lambda: p3d.loss.mesh_edge_loss(mesh),
            lambda: p3d.loss.mesh_normal_consistency(mesh), lambda: p3d.loss.mesh_laplacian_smoothing(mesh, "uniform"))


def torch_terms(mesh, xs, ys):
    v = mesh.verts_packed()

    def chamfer():
        d2 = torch.cdist(xs, ys) ** 2
        return d2.min(2)[0].mean() + d2.min(1)[0].mean()

    def normal():
        pa = v[quads[:, 0]]
        eb, ec, ed = v[quads[:, 1]] - pa, v[quads[:, 2]] - pa, v[quads[:, 3]] - pa
        return (1 - torch.cosine_similarity(torch.cross(ec, eb, dim=1), -torch.cross(ed, eb, dim=1), dim=1)).mean()

    def lap():
        nb = torch.zeros_like(v).index_add(0, edges[:, 0], v[edges[:, 1]]).index_add(0, edges[:, 1], v[edges[:, 0]])
        return (nb / deg[:, None] - v).norm(dim=1).mean()

    return chamfer, lambda: ((v[edges[:, 0]] - v[edges[:, 1]]).norm(dim=1) ** 2).mean(), normal, lap


WEIGHTS = (1.0, 1.0, 0.01, 0.1)


def step(terms, parts=(0, 1, 2, 3)):
    """One iteration with the terms `parts` (the chamfer term alone still needs both samplings)."""
    mesh = Meshes(verts=[base + offset], faces=[faces])
    xs, ys = (samples(target), samples(mesh)) if 0 in parts else (None, None)
    fns = terms(mesh, xs, ys)
    t = [fns[i]() for i in parts]
    loss = sum(WEIGHTS[i] * x.reshape(()) for i, x in zip(parts, t))
    return torch.autograd.grad(loss, [offset])[0], t


def median_us(fn):
    for _ in range(a.warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)]
    for e0, e1 in ev:
        e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return sorted(e0.elapsed_time(e1) for e0, e1 in ev)[a.reps // 2] * 1e3


g_hip, t_hip = step(hip_terms)
g_torch, t_torch = step(torch_terms)
print("terms (chamfer, edge, normal, laplacian; different samples): hip %s  torch %s"
      % ([round(float(x), 6) for x in t_hip], [round(float(x), 6) for x in t_torch]))
print("one fit iteration, %d + %d samples (%s draws), forward + backward, median of %d:"
      % (S, S, "kernel" if a.sampler else "torch", a.reps))
for name, terms in (("HIP operators", hip_terms), ("torch ops", torch_terms)):
    print("  %-14s %8.1f us" % (name, median_us(lambda: step(terms))))
for i, tag in enumerate(("chamfer", "edge", "normal", "laplacian")):
    print("  %-10s alone%s: HIP %8.1f us   torch %8.1f us"
          % (tag, " (with both samplings)" if i == 0 else "", median_us(lambda: step(hip_terms, (i,))),
             median_us(lambda: step(torch_terms, (i,)))))
print("  sampling alone: %.1f us" % median_us(lambda: (samples(target), samples(Meshes(verts=[base + offset], faces=[faces])))))

if a.loop:
    from acfm_video_3d_reconstruction_amd import template_fit
    v, f = base.cpu().numpy(), faces.cpu().numpy()
    tv = target.verts_list()[0].cpu().numpy()
    print("the whole loop, %d iterations (wall time; per iteration; scaled to 2000 iterations):" % a.loop)
    for name, kw in (("eager, torch draws", {}), ("eager, kernel draws", {"sampler": SurfaceSampler(seed=0)}),
                     ("replayed, kernel draws", {"sampler": SurfaceSampler(seed=0), "use_graph": True})):
        template_fit.fit_verts_to_mesh(v, f, tv, f, n_iter=min(a.loop, 20), num_samples=S, device=d, **kw)    # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        template_fit.fit_verts_to_mesh(v, f, tv, f, n_iter=a.loop, num_samples=S, device=d, **kw)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print("  %-24s %8.3f s   %8.1f us / iteration   %6.2f s / 2000" % (name, dt, dt / a.loop * 1e6, dt / a.loop * 2000))
