"""Generates uv_atlas.npz FROM THE REFERENCE ITSELF (data only; no reference source is copied).

Run in the authoring container only (needs /root/reference, read-only):

    python tests/golden/make_golden_uv_atlas.py

It imports the reference's utils/mesh.py (after restoring the ``np.float`` alias numpy 2 dropped, which that file still
uses) and stores
  verts [642,3] f64, faces [1280,3] i64   the symmetric level-3 sphere: make_symmetric(create_sphere(3)); faces[:656]
                                          are the 32 independent + 624 right-hand faces the symmetric texture samples
  num_indept_faces = 32, num_sym_faces = 624
  sampler_t2 [656,2,2,2], sampler_t6 [656,6,6,2] f64   compute_uvsampler(verts, faces[:656], tex_size)
  uvimage [2,3,32,64] f32                 a fixed N(0, 1) image
  atlas_t2 [2,1280,2,2,3] f32             mesh_net.py:169-176 on that image with sampler_t2, torch-CPU float32
"""
import os
import sys

import numpy as np
import torch

REF = "/root/reference/multiframe"
OUT = os.path.dirname(os.path.abspath(__file__))

np.float = float
sys.path.insert(0, REF)
from utils import mesh as ref_mesh  # noqa: E402  (the reference's own module)


def main():
    verts, faces = ref_mesh.create_sphere(3)
    verts, faces, _, _, n_indept, n_sym = ref_mesh.make_symmetric(verts, faces)
    assert (n_indept, n_sym, faces.shape[0]) == (32, 624, 1280)
    nf = n_indept + n_sym
    samplers = {T: ref_mesh.compute_uvsampler(verts, faces[:nf], tex_size=T) for T in (2, 6)}
    uvimage = torch.from_numpy(np.random.default_rng(20240607).standard_normal((2, 3, 32, 64)).astype(np.float32))

    # the operations of mesh_net.py:155 and 169-176 with symmetric=True, on torch-CPU float32
    T, B = 2, uvimage.shape[0]
    grid = torch.tensor(samplers[T], dtype=torch.float32).reshape(1, nf, T * T, 2)
    sampled = torch.nn.functional.grid_sample(uvimage, grid.repeat(B, 1, 1, 1), align_corners=True)   # [B,3,nf,T*T]
    tex = sampled.reshape(B, 3, nf, T, T).permute(0, 2, 3, 4, 1)
    tex = (torch.tanh(tex) + 1) / 2
    atlas = torch.cat([tex, tex[:, -n_sym:]], 1)
    assert tuple(atlas.shape) == (2, 1280, 2, 2, 3)

    path = os.path.join(OUT, "uv_atlas.npz")
    np.savez_compressed(path, verts=np.asarray(verts, np.float64), faces=np.asarray(faces, np.int64),
                        num_indept_faces=np.int64(n_indept), num_sym_faces=np.int64(n_sym),
                        sampler_t2=samplers[2].astype(np.float64), sampler_t6=samplers[6].astype(np.float64),
                        uvimage=uvimage.numpy(), atlas_t2=atlas.numpy())
    print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
