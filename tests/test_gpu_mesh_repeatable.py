"""GPU: the Laplacian-smoothing loss and the edge-rigidity loss (csrc/acfm_mesh.hip) repeat their bits from launch to
launch.  They used to add with float atomics in arrival order (waves into LDS, workgroups into the scalar) and did not
agree with themselves in the last bit, which tests that compare two steps bit for bit met now and then.  Pinned here
where it can go wrong: one mesh, two (a two-term sum is order-free by itself), five (more than two partial sums); the
rigidity loss also at the largest batch its one-workgroup kernel takes (24576 edges; larger batches keep the atomic and
are not claimed, nor is the Laplacian's global-atomic path).  The values are pinned against float64 in
test_gpu_mesh_priors.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu

LAUNCHES = 40


def _d():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _batch(meshes, n, d):
    from acfm_video_3d_reconstruction_amd.pytorch3d_shim.structures import Meshes
    g = torch.Generator().manual_seed(70 + n)
    v0 = torch.tensor(meshes["bird_v"])
    v = (v0[None] * (1 + 0.01 * torch.randn(n, v0.shape[0], 3, generator=g))).to(d)
    f = torch.tensor(meshes["bird_f"]).long().to(d)[None].repeat(n, 1, 1)
    ms = Meshes(verts=v, faces=f)
    return v.reshape(-1, 3).contiguous(), ms.faces_packed(), ms.edges_packed(), v0.shape[0], f.shape[1]


def _distinct(fn):
    return {fn().item().hex() for _ in range(LAUNCHES)}


@pytest.mark.parametrize("n", [1, 2, 5])
def test_laplacian_loss_repeats_its_bits(meshes, n):
    """The per-mesh LDS path (cot weights, equal-sized meshes: what the trainers call)."""
    from acfm_video_3d_reconstruction_amd import ops
    vp, fp, ep, V, F = _batch(meshes, n, _d())
    w = torch.full((vp.shape[0],), 1.0 / V, device=vp.device)
    seen = _distinct(lambda: ops.laplacian_smoothing_sum(vp, fp, w, 0, V, F))
    assert len(seen) == 1, seen


@pytest.mark.parametrize("n", [1, 2, 12])
def test_rigidity_loss_repeats_its_bits(meshes, n):
    """12 meshes are 23040 edges: the largest batch of this mesh that the one-workgroup kernel (<= 24576 edges) takes."""
    from acfm_video_3d_reconstruction_amd import ops
    vp, fp, ep, V, F = _batch(meshes, n, _d())
    assert ep.shape[0] == 1920 * n <= 24576
    vt = (vp * 1.05).contiguous()
    seen = _distinct(lambda: ops.edge_rigidity_sum(vp, ep, vt, ep, V))
    assert len(seen) == 1, seen
