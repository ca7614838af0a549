"""Template deformation solve.

The reference (multiframe/main.py:586-609, nnutils/predictor.py:260-276, 313-315) builds, for
every frame, M = L^T L + A^T A and b = L^T L v + A^T (A v + delta) and calls torch.cholesky +
cholesky_solve on B*T identical 642x642 systems.  Algebraically b = M v + A^T delta, so

        pred_v_n = v + P delta_n,      P = M^-1 A^T   (V x K_h)

P depends only on the handle weights (lbs) and on the no-grad Laplacian of the mean shape; both
are learned (mesh_net.py:480, 543), so it is rebuilt ONCE per optimiser step: on the GPU by the
blocked fp64 Cholesky of csrc/acfm_solve.hip (ops.deform_solve: more accurate than the
reference's own fp32 Cholesky), and applied per frame as a [V x K_h] . [K_h x 3]
product (ops.deform_apply).  Gradients: d delta_n = P^T g_n, d v = sum_n g_n (L is a constant,
geom_utils.py:245), d lbs through the saved factor (acfm_deform_solve_backward).
"""
import torch
from torch import nn

from .nnutils import geom_utils


class _OneMesh:
    """The 4-method view of a single mesh that geom_utils.mesh_laplacian needs."""

    def __init__(self, verts, faces):
        self._v, self._f, self.device = verts, faces, verts.device

    def isempty(self):
        return False

    def verts_packed(self):
        return self._v

    def faces_packed(self):
        return self._f


def handle_matrix(lbs_logits):
    """MeshNet.get_lbs().permute(1, 0) (mesh_net.py:597-599, main.py:586): A [K_h, V]."""
    return torch.softmax(lbs_logits, dim=0).permute(1, 0)


def solve_matrix(L, A):
    """P = (L^T L + A^T A)^-1 A^T in fp64 via torch.linalg (host tensors / cross-check of the
    native kernel; main.py:605-608 collapsed)."""
    L64, A64 = L.double(), A.double()
    M = L64.t() @ L64 + A64.t() @ A64
    u = torch.linalg.cholesky(M)
    return torch.cholesky_solve(A64.t(), u)


def _solve(L, lbs_logits):
    if lbs_logits.is_cuda:
        from . import ops
        return ops.deform_solve(L, lbs_logits)
    return solve_matrix(L, handle_matrix(lbs_logits)).float()


class DeformSolver(nn.Module):
    """mean_v / lbs_logits may be nn.Parameters (learned, as in the reference) or plain tensors.
    symmetry=(num_indept, num_sym): the reference's symmetric template (mesh_net.py:462-484).  mean_v then holds the
    num_indept + num_sym rows on the mirror plane and right of it, as the reference's parameter does, and every reader
    of the geometry goes through mean_shape(), which appends the mirrored right rows (template.symmetrize)."""

    def __init__(self, mean_v, faces, lbs_logits, method="cot", symmetry=None):
        super().__init__()
        self.method = method
        self.symmetry = None
        if symmetry is not None:
            n_indept, n_sym = int(symmetry[0]), int(symmetry[1])
            if n_indept < 0 or n_sym < 0 or mean_v.shape[0] != n_indept + n_sym:
                raise ValueError("symmetry = (%d, %d): mean_v must have num_indept + num_sym = %d rows, got %d"
                                 % (n_indept, n_sym, n_indept + n_sym, mean_v.shape[0]))
            if int(faces.max()) + 1 != n_indept + 2 * n_sym:
                raise ValueError("symmetry = (%d, %d): the faces index %d vertices, not num_indept + 2 num_sym = %d"
                                 % (n_indept, n_sym, int(faces.max()) + 1, n_indept + 2 * n_sym))
            self.symmetry = (n_indept, n_sym)
        if isinstance(mean_v, nn.Parameter):
            self.mean_v = mean_v
        else:
            self.register_buffer("mean_v", mean_v.detach().clone())
        self.register_buffer("faces", faces.detach().clone().long())
        if isinstance(lbs_logits, nn.Parameter):
            self.lbs = lbs_logits
        else:
            self.register_buffer("lbs", lbs_logits.detach().clone())
        self._P = None
        self._L = None

    def mean_shape(self):
        """The full [V,3] mean shape (MeshNet.get_mean_shape, mesh_net.py:593-595): mean_v itself without symmetry, else
        its rows followed by the mirrored right rows, with the autograd path back to the half parameter."""
        if self.symmetry is None:
            return self.mean_v
        from . import template
        return template.symmetrize(self.mean_v, self.symmetry[1])

    def laplacian(self, mean_v=None):
        v = (self.mean_shape() if mean_v is None else mean_v).detach()
        return geom_utils.mesh_laplacian(_OneMesh(v, self.faces), self.method)

    def refresh(self, mean_v=None):
        """Call after lbs or the mean shape (which defines L) changed, i.e. once per optimiser
        step: the next solve_matrix() rebuilds L and re-factorises.  mean_v: the FULL shape, where the caller has
        formed it already."""
        self._P = None
        self._L = self.laplacian(mean_v)

    def solve_matrix(self):
        """P [V,K_h]; one factorisation per refresh().  With lbs requiring grad (and grad mode on)
        the factorisation is part of the autograd graph of this step."""
        if self._L is None:
            self._L = self.laplacian()
        if self.lbs.requires_grad and torch.is_grad_enabled():
            P = _solve(self._L, self.lbs)
            self._P = P.detach()
            return P
        if self._P is None:
            with torch.no_grad():
                self._P = _solve(self._L, self.lbs)
        return self._P

    def forward(self, delta, mean_override=None):
        """delta [N,K_h,3] handle offsets -> deformed verts [N,V,3] (delta = 0: the mean shape)."""
        mean = self.mean_shape() if mean_override is None else mean_override
        P = self.solve_matrix()
        if delta.is_cuda:
            from . import ops
            return ops.deform_apply(mean, P, delta)   # f32 MFMA kernels (csrc/acfm_deform.hip)
        return mean[None] + torch.matmul(P[None], delta)  # host tensors: CPU-side tests of the algebra


def deform_reference_formula(lbs_logits, mean_v, delta, L):
    """The reference's expression, term by term (main.py:586-609), on device tensors;
    for tests and for callers that want the literal formulation."""
    A = handle_matrix(lbs_logits)
    nb = delta.shape[0]
    A_b = A[None].repeat(nb, 1, 1)
    mean_b = mean_v[None].repeat(nb, 1, 1)
    delta_v = A_b.bmm(mean_b) + delta
    L_b = L[None].repeat(nb, 1, 1)
    d = torch.bmm(L_b, mean_b)
    A_augm = L_b.permute(0, 2, 1).matmul(L_b) + A_b.permute(0, 2, 1).matmul(A_b)
    b = L_b.permute(0, 2, 1) @ d + A_b.permute(0, 2, 1) @ delta_v
    u = torch.linalg.cholesky(A_augm)
    return torch.cholesky_solve(b, u)
