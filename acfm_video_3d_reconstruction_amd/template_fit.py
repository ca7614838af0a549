"""Fitting a template to a target mesh: the loop of utils/geometry.py:75-137 (fit_verts_to_mesh) on this package's
operators, optionally as one captured iteration that is replayed.

    verts = fit_verts_to_mesh(sphere_verts, sphere_faces, target_verts, target_faces,
                              sampler=SurfaceSampler(seed=0), use_graph=True)

An iteration samples both surfaces, sums chamfer + edge length + normal consistency + cot Laplacian, and moves a
per-vertex offset by SGD with momentum.  With a surface_sampling.SurfaceSampler every draw is a kernel whose counter
lives on the device, so the captured iteration draws fresh samples at every replay; without one the draws are torch's
(global generator), which a graph cannot contain: use_graph then needs a sampler."""
import numpy as np
import torch

from . import pytorch3d_shim as p3d
from .pytorch3d_shim.structures import Meshes

TERMS = ("chamfer", "edge", "normal", "laplacian")


def _as_tensor(a, dtype, device):
    return torch.as_tensor(np.asarray(a)).to(device=device, dtype=dtype).contiguous()


def fit_verts_to_mesh(verts, faces, trg_verts, trg_faces, n_iter=2000, num_samples=5000,
                      weights=(1.0, 1.0, 0.01, 0.1), sampler=None, use_graph=False, device=None, n_eager=3,
                      return_history=False):
    """verts [V,3], faces [F,3]: the template; trg_verts, trg_faces: the target (arrays or tensors) -> the fitted
    vertices, numpy [V,3], in the target's own frame.
    The target is centred and scaled into [-1, 1] by its largest coordinate; an offset per template vertex, zero at
    the start, is learned for n_iter steps of SGD (lr 1, momentum 0.9) on
        weights . (chamfer of num_samples surface points a side, edge length, normal consistency, cot Laplacian);
    the result is scaled and moved back.
      sampler    a SurfaceSampler: both draws of every iteration are its counter-based ones (2 n_iter draws in all);
                 None: torch.multinomial / torch.rand.
      use_graph  run n_eager iterations eagerly, capture the next one -- both draws, the four terms, the backward and
                 the momentum update -- into a hipGraph and replay it for the rest.  GPU and a sampler only.
      device     default: the current GPU.  A host device runs the shim's host formulations (slow; for tests).
      return_history  also return the four terms of every iteration, numpy [n_iter, 4] in the order of TERMS.
    Eager and replayed runs differ only in the order of the float atomic additions of the backward kernels."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    n_iter, S = int(n_iter), int(num_samples)
    if use_graph and (device.type != "cuda" or sampler is None):
        raise ValueError("fit_verts_to_mesh: use_graph needs GPU tensors and a sampler (torch's draws cannot be captured)")
    base = _as_tensor(verts, torch.float32, device)
    tri = _as_tensor(faces, torch.int64, device)
    target = _as_tensor(trg_verts, torch.float32, device)
    target_tri = _as_tensor(trg_faces, torch.int64, device)
    centre = target.mean(0)
    target = target - centre
    scale = target.abs().max()
    target_mesh = Meshes(verts=[target / scale], faces=[target_tri])

    offset = torch.zeros_like(base, requires_grad=True)
    velocity = torch.zeros_like(base)
    terms = torch.zeros(4, dtype=torch.float32, device=device)
    w = [float(x) for x in weights]

    def iteration():
        mesh = Meshes(verts=[base + offset], faces=[tri])
        there = p3d.ops.sample_points_from_meshes(target_mesh, S, sampler=sampler)
        here = p3d.ops.sample_points_from_meshes(mesh, S, sampler=sampler)
        t = (p3d.loss.chamfer_distance(there, here)[0], p3d.loss.mesh_edge_loss(mesh),
             p3d.loss.mesh_normal_consistency(mesh), p3d.loss.mesh_laplacian_smoothing(mesh, method="cot"))
        t = [x.reshape(()) for x in t]
        loss = (t[0] * w[0] + t[1] * w[1]) + (t[2] * w[2] + t[3] * w[3])
        grad, = torch.autograd.grad(loss, [offset])
        with torch.no_grad():                   # SGD, lr 1, momentum 0.9 (the first step's velocity is the gradient)
            velocity.mul_(0.9).add_(grad)
            offset.sub_(velocity)
            terms.copy_(torch.stack([x.detach() for x in t]))

    history = torch.zeros((n_iter, 4), dtype=torch.float32, device=device) if return_history else None

    def run(step, i):
        step()
        if history is not None:
            history[i].copy_(terms)

    done = 0
    if use_graph and n_iter > n_eager:
        side = torch.cuda.Stream(device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):           # state, tables, scratch and the allocator exist before the capture
            for done in range(1, n_eager + 1):
                run(iteration, done - 1)
        torch.cuda.current_stream(device).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):           # records, runs nothing: the draw counter stays where it is
            iteration()
        for i in range(done, n_iter):
            run(graph.replay, i)
    else:
        for i in range(n_iter):
            run(iteration, i)
    out = ((base + offset.detach()) * scale + centre).cpu().numpy()
    if return_history:
        return out, history.cpu().numpy()
    return out
