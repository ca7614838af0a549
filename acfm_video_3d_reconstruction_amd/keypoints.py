"""Keypoint supervision: the annotated-keypoint head of the trainers and the predictor.

`KeypointHead` is what multiframe/main.py:503-511 / 690-696, monocular/main.py:203-232 and predictor.py:258, 281-282,
352-355 do with `vert2kp`: `kp_verts = softmax(vert2kp) @ verts`, `kp_pred = project_points(kp_verts, cams)`,
`kp_l2_loss(kp_pred, kps)`, and the entropy prior `entropy_loss(softmax(vert2kp))`.  On the GPU these are
ops.kp_weights + ops.kp_head (csrc/acfm_keypoints.hip): two launches forward, three or four back.  On host tensors the
same reference lines run as torch ops; they are the definition the kernels are tested against."""
import collections
import weakref

import torch
from torch import nn

from . import ops
from .nnutils import loss_utils
from .nnutils.geom_utils import hamilton_product

KeypointOutput = collections.namedtuple("KeypointOutput", ["kp_verts", "kp_pred", "loss", "kp_err"])


def project_xy_host(X, cam):
    """geom_utils.orthographic_proj (geom_utils.py:48-59, quat_rotate :134-152) as torch ops of any dtype and device:
    X [B,P,3], cam [B,7] -> [B,P,2]."""
    q = cam[:, None, -4:] * (X[[0], :, :][:, :, [0]] * 0 + 1)
    q_conj = torch.cat([q[:, :, [0]], -1 * q[:, :, 1:4]], dim=-1)
    X4 = torch.cat([X[:, :, [0]] * 0, X], dim=-1)
    X_rot = hamilton_product(q, hamilton_product(X4, q_conj))[:, :, 1:4]
    return cam[:, 0].reshape(-1, 1, 1) * X_rot[:, :, :2] + cam[:, 1:3].reshape(cam.shape[0], 1, -1)


def pixel_error(kp_pred, kp_gt, img_size):
    """evaluate.py:156-158: distance in pixels between predicted and annotated keypoints, [N,K]."""
    return torch.norm((kp_pred + 1) * img_size / 2 - (kp_gt[..., :2] + 1) * img_size / 2, dim=2)


# KeypointHead -> (key, A, entropy) of its last weights() call on the GPU.  Kept beside the module, not in it: A is a
# non-leaf tensor, which copy.deepcopy / pickling of the module must never meet; a copy starts without an entry.
_WEIGHTS = weakref.WeakKeyDictionary()


class KeypointHead(nn.Module):
    """vert2kp: [K,V] logits, a tensor or an nn.Parameter (mesh_net.py:504-519 builds and learns it)."""

    def __init__(self, vert2kp):
        super().__init__()
        if vert2kp.dim() != 2:
            raise ValueError("KeypointHead: vert2kp [K,V] expected, got %s" % (tuple(vert2kp.shape),))
        if isinstance(vert2kp, nn.Parameter):
            self.vert2kp = vert2kp
        else:
            self.register_buffer("vert2kp", vert2kp)

    def weights(self):
        """(A, entropy): softmax(vert2kp, 1) and entropy_loss(A).  One ops.kp_weights call serves every use until the
        logits change (their autograd version) or a backward pass has gone through it (which frees its graph)."""
        x = self.vert2kp
        if not x.is_cuda:
            A = torch.softmax(x, dim=1)
            return A, loss_utils.entropy_loss(A)
        # (the capture id: tensors made while a hipGraph is captured serve that capture only)
        key = (x.data_ptr(), x._version, tuple(x.shape), torch.is_grad_enabled() and x.requires_grad,
               ops._capture_id(x.device))
        hit = _WEIGHTS.get(self)
        if hit is None or hit[0] != key:
            A, ent = ops.kp_weights(x)
            if A.grad_fn is not None:
                # (a weak reference: the node must not keep the module -- and with it this very entry -- alive)
                me = weakref.ref(self)

                def drop(*_):
                    head = me()
                    if head is not None:
                        _WEIGHTS.pop(head, None)
                A.grad_fn.register_hook(drop)
            hit = _WEIGHTS[self] = (key, A, ent)
        return hit[1], hit[2]

    def entropy(self):
        return self.weights()[1]

    def forward(self, verts, cams, kp_gt=None, reduction='none', img_size=None):
        """verts [Nv,V,3], cams [N,7], kp_gt [Ng,K,3] or None; camera n sees vertices n % Nv and ground truth n % Ng
        (the G hypotheses of a frame share both: pass them unrepeated).  -> KeypointOutput(kp_verts [Nv,K,3],
        kp_pred [N,K,2], loss = kp_l2_loss(kp_pred, kp_gt, reduction) or None, kp_err [N,K] pixels (with kp_gt and
        img_size) or None)."""
        if reduction not in ('none', 'mean'):
            raise ValueError("KeypointHead: reduction 'none' or 'mean', got %r" % (reduction,))
        N, Nv = cams.shape[0], verts.shape[0]
        Ng = 1 if kp_gt is None else kp_gt.shape[0]
        if Nv < 1 or Ng < 1 or N % Nv or N % Ng:
            raise ValueError("KeypointHead: %d cameras cannot share %d rows of vertices and %d of ground truth"
                             % (N, Nv, Ng))
        A, _ = self.weights()
        want_err = kp_gt is not None and img_size is not None
        if A.is_cuda:
            kp_verts, kp_pred, loss, err = ops.kp_head(A, verts, cams, kp_gt, img_size, want_err)
            if loss is not None and reduction == 'mean':
                loss = loss.mean()
            return KeypointOutput(kp_verts, kp_pred, loss, err)
        kp_verts = torch.matmul(A, verts)
        kp_pred = project_xy_host(kp_verts.repeat(N // Nv, 1, 1), cams)
        loss = err = None
        if kp_gt is not None:
            gt = kp_gt.repeat(N // Ng, 1, 1)
            loss = loss_utils.kp_l2_loss(kp_pred, gt, reduction=reduction)
            if want_err:
                err = pixel_error(kp_pred, gt, img_size).detach()
        return KeypointOutput(kp_verts, kp_pred, loss, err)
