"""Surface samples of packed meshes drawn on the device (csrc/acfm_sample.hip: k_surface_cdf, k_surface_sample,
k_surface_bwd_lds / k_surface_bwd_scatter).  surface_sampling.surface_sample_host is the definition."""
import ctypes

import torch

from .. import _lib
from .base import _f32c, _i64c


class _SurfaceSample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, state, verts_packed, faces_packed, first_dev, first_host, S, vpm):
        _lib.require_gpu(state, verts_packed, faces_packed, first_dev)
        if state.dtype != torch.int64 or tuple(state.shape) != (2,) or not state.is_contiguous():
            raise ValueError("sample_surface: state must be a contiguous int64 [2] tensor (seed, draw)")
        v, f = _f32c(verts_packed), _i64c(faces_packed)
        P, F, N = v.shape[0], f.shape[0], first_dev.shape[0] - 1
        points = torch.empty((N, S, 3), dtype=torch.float32, device=v.device)
        face_idx = torch.empty((N, S), dtype=torch.int32, device=v.device)
        uv = torch.empty((N, S, 2), dtype=torch.float32, device=v.device)
        nbytes = int(_lib.lib().acfm_surface_sample_workspace_bytes(N, F))
        ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=v.device)
        host = None if first_host is None else ctypes.c_void_p(first_host.data_ptr())
        _lib.call("acfm_surface_sample", v.device, state, v, f if F else None, first_dev, host, N, S, P, F, points,
                  face_idx, uv, ws, nbytes)
        ctx.save_for_backward(f, face_idx, uv)
        ctx.cfg = (N, S, P, F, int(vpm))
        ctx.mark_non_differentiable(face_idx, uv)
        return points, face_idx, uv

    @staticmethod
    def backward(ctx, gp, _gf, _guv):
        f, face_idx, uv = ctx.saved_tensors
        N, S, P, F, vpm = ctx.cfg
        g = _f32c(gp)
        gv = torch.empty((P, 3), dtype=torch.float32, device=g.device)
        _lib.call("acfm_surface_sample_backward", g.device, g, face_idx, uv, f if F else None, N, S, P, F, vpm, gv)
        return None, gv, None, None, None, None, None


def sample_surface_uv(state, verts_packed, faces_packed, first_idx, num_samples, verts_per_mesh=0):
    """sample_surface, and the (u, v) of every sample: -> (points [N,S,3], face_idx [N,S] i32, uv [N,S,2])."""
    if verts_packed.dim() != 2 or verts_packed.shape[1] != 3 or verts_packed.shape[0] == 0:
        raise ValueError("sample_surface: verts_packed [P,3] with P >= 1 expected, got %s" % (tuple(verts_packed.shape),))
    if faces_packed.dim() != 2 or faces_packed.shape[1] != 3:
        raise ValueError("sample_surface: faces_packed [F,3] expected, got %s" % (tuple(faces_packed.shape),))
    if first_idx.dim() != 1 or first_idx.shape[0] < 2:
        raise ValueError("sample_surface: first_idx [N+1] with N >= 1 expected, got %s" % (tuple(first_idx.shape),))
    if int(num_samples) <= 0:
        raise ValueError("sample_surface: num_samples must be positive")
    first_host = first_dev = None
    if first_idx.is_cuda:
        first_dev = _i64c(first_idx)
    else:                                   # host table: checked there, uploaded once per (values, device)
        first_host = _i64c(first_idx)
        vals = first_host.tolist()
        if any(b < a for a, b in zip([0] + vals, vals)) or vals[-1] > faces_packed.shape[0]:
            raise ValueError("sample_surface: first_idx must be non-decreasing within [0, F], got %s" % (vals,))
        first_dev = _lib.const(vals, verts_packed.device, torch.int64)
    return _SurfaceSample.apply(state, verts_packed, faces_packed, first_dev, first_host, int(num_samples),
                                int(verts_per_mesh))


def sample_surface(state, verts_packed, faces_packed, first_idx, num_samples, verts_per_mesh=0):
    """num_samples points on the surface of each of N packed meshes, drawn on the GPU: faces with replacement in
    proportion to their area, then a uniform point of each (PyTorch3D's sample_points_from_meshes; the distribution,
    not its random stream).  -> (points [N,S,3] f32, face_idx [N,S] i32: the row of faces_packed, -1 for a mesh
    without area, whose points are 0).
      state        int64 [2] = (seed, draw) on the device (surface_sampling.SurfaceSampler.state_on); the call uses
                   the draw and leaves it one higher, in stream order: a captured call draws afresh at every replay.
      verts_packed [P,3], faces_packed [F,3] (any integer or float dtype, packed vertex ids).
      first_idx    [N+1] int64: mesh m = faces [first_idx[m], first_idx[m+1]).  A HOST tensor is checked (ValueError
                   unless non-decreasing within [0, F]) and uploaded once; a device tensor is clamped by the kernels.
      verts_per_mesh  > 0: N equal-sized meshes one after the other (the backward then adds per mesh in LDS).
    Areas are quantised to 24 bits of the mesh's largest face: a face below 2^-24 of it is never drawn.
    Differentiable in verts_packed only; the gradient sums float atomics and is not bit-reproducible (as
    chamfer_nearest's)."""
    return sample_surface_uv(state, verts_packed, faces_packed, first_idx, num_samples, verts_per_mesh)[:2]
