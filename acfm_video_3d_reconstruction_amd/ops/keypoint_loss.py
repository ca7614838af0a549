"""Keypoint supervision and the camera loss (csrc/acfm_keypoints.hip)."""
import torch

from .. import _lib
from .base import _f32c


KP_MAX_K = 64          # keypoints: one lane each
KP_MAX_V = 65535
KP_MAX_N = 65535


def _kp_f32(name, *tensors):
    for t in tensors:
        if t is not None and t.dtype != torch.float32:
            raise ValueError("%s: float32 only, got %s" % (name, t.dtype))


def _kp_limits(name, K, V, N=0, Nv=1, Ng=1):
    if not 1 <= K <= KP_MAX_K:
        raise ValueError("%s: 1 <= K <= %d keypoints, got K = %d" % (name, KP_MAX_K, K))
    if not 1 <= V <= KP_MAX_V:
        raise ValueError("%s: 1 <= V <= %d vertices, got V = %d" % (name, KP_MAX_V, V))
    if N > KP_MAX_N:
        raise ValueError("%s: N <= %d cameras, got N = %d" % (name, KP_MAX_N, N))
    if N and (Nv < 1 or N % Nv):
        raise ValueError("%s: N %% Nv == 0: %d cameras do not share %d rows of vertices evenly" % (name, N, Nv))
    if N and (Ng < 1 or N % Ng):
        raise ValueError("%s: N %% Ng == 0: %d cameras do not share %d rows of ground truth evenly" % (name, N, Ng))


class _KpWeights(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits):
        ctx.set_materialize_grads(False)
        x = _f32c(logits)
        K, V = x.shape
        A = torch.empty_like(x)
        entropy = torch.empty((), dtype=torch.float32, device=x.device)
        stats = torch.empty((K, 2), dtype=torch.float32, device=x.device)
        _lib.call("acfm_kp_weights_forward", x.device, x, K, V, A, entropy, stats)
        ctx.save_for_backward(x, A, stats)
        return A, entropy

    @staticmethod
    def backward(ctx, gA, ge):
        if gA is None and ge is None:
            return None
        x, A, stats = ctx.saved_tensors
        K, V = x.shape
        gA = None if gA is None else _f32c(gA)
        ge = None if ge is None else _f32c(ge)
        gx = torch.empty_like(x)
        _lib.call("acfm_kp_weights_backward", x.device, x, A, stats, gA, ge, K, V, gx)
        return gx


def kp_weights(logits):
    """vert2kp logits [K,V] -> (A = softmax(logits, 1) [K,V], entropy_loss(A) as a scalar) from one launch each way
    (mesh_net.py:504-519's softmax, loss_utils.py:330-338).  The entropy is evaluated from the log-softmax, so it and
    its gradient stay finite where A underflows to 0 (the reference's A * log(A) is NaN there)."""
    if logits.dim() != 2:
        raise ValueError("kp_weights: logits [K,V] expected, got %s" % (tuple(logits.shape),))
    _kp_f32("kp_weights", logits)
    _kp_limits("kp_weights", logits.shape[0], logits.shape[1])
    _lib.require_gpu(logits)
    return _KpWeights.apply(logits)


class _KpHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, A, verts, cams, kp_gt, img_size, want_err):
        ctx.set_materialize_grads(False)
        a, v, c = _f32c(A), _f32c(verts), _f32c(cams)
        g = None if kp_gt is None else _f32c(kp_gt)
        K, V = a.shape
        Nv, N, Ng = v.shape[0], c.shape[0], (1 if g is None else g.shape[0])
        dev = a.device
        kp_verts = torch.empty((Nv, K, 3), dtype=torch.float32, device=dev)
        kp_pred = torch.empty((N, K, 2), dtype=torch.float32, device=dev)
        loss = None if g is None else torch.empty((N,), dtype=torch.float32, device=dev)
        err = torch.empty((N, K), dtype=torch.float32, device=dev) if want_err else None
        _lib.call("acfm_kp_head_forward", dev, a, v, c, g, K, V, N, Nv, Ng, float(img_size or 0.0), kp_verts, kp_pred,
                  loss, err)
        ctx.save_for_backward(a, v, c, g, kp_verts, kp_pred)
        if err is not None:
            ctx.mark_non_differentiable(err)
        return kp_verts, kp_pred, loss, err

    @staticmethod
    def backward(ctx, g_kpv, g_pred, g_loss, _g_err):
        a, v, c, gt, kp_verts, kp_pred = ctx.saved_tensors
        need = ctx.needs_input_grad
        if not any(need[:3]) or (g_kpv is None and g_pred is None and g_loss is None):
            return None, None, None, None, None, None
        K, V = a.shape
        Nv, N, Ng = v.shape[0], c.shape[0], (1 if gt is None else gt.shape[0])
        dev = a.device
        g_kpv, g_pred, g_loss = [None if t is None else _f32c(t) for t in (g_kpv, g_pred, g_loss)]
        gA = torch.empty_like(a) if need[0] else None
        gv = torch.empty_like(v) if need[1] else None
        gc = torch.empty_like(c) if need[2] else None
        nb = int(_lib.lib().acfm_kp_head_workspace_bytes(K, Nv))
        ws = torch.empty((nb,), dtype=torch.uint8, device=dev)
        _lib.call("acfm_kp_head_backward", dev, a, v, c, gt, kp_verts, kp_pred, g_loss, g_pred, g_kpv, K, V, N, Nv, Ng,
                  gA, gv, gc, ws, nb)
        return gA, gv, gc, None, None, None


def kp_head(A, verts, cams, kp_gt=None, img_size=None, want_err=False):
    """The keypoint head in one launch (two or three back): A [K,V] (kp_weights), verts [Nv,V,3], cams [N,7],
    kp_gt [Ng,K,3] (x, y, visibility) or None -> (kp_verts [Nv,K,3] = A @ verts, kp_pred [N,K,2] = its projection --
    the bits of project_xy(kp_verts, cams) --, loss [N] = kp_l2_loss(kp_pred, kp_gt, reduction='none') or None,
    kp_err [N,K] = evaluate.py:156-158's pixel error (want_err=True, needs img_size; no gradient) or None).
    Camera n reads vertices n % Nv and ground truth n % Ng: the G hypotheses of a frame share both, as the reference's
    repeat(G, 1, 1) copies would.  Gradients to A, verts and cams; d|x| at 0 is 0."""
    if A.dim() != 2 or verts.dim() != 3 or verts.shape[2] != 3 or verts.shape[1] != A.shape[1] \
            or cams.dim() != 2 or cams.shape[1] != 7:
        raise ValueError("kp_head: A [K,V], verts [Nv,V,3], cams [N,7] expected, got %s, %s, %s"
                         % (tuple(A.shape), tuple(verts.shape), tuple(cams.shape)))
    K, V = A.shape
    if kp_gt is not None and (kp_gt.dim() != 3 or kp_gt.shape[1] != K or kp_gt.shape[2] != 3):
        raise ValueError("kp_head: kp_gt [Ng,%d,3] expected, got %s" % (K, tuple(kp_gt.shape)))
    if want_err and (kp_gt is None or img_size is None):
        raise ValueError("kp_head: want_err needs kp_gt and img_size")
    if cams.shape[0] == 0:          # (the library launches nothing for N == 0, kp_verts included)
        raise ValueError("kp_head: at least one camera, got cams %s" % (tuple(cams.shape),))
    _kp_f32("kp_head", A, verts, cams, kp_gt)
    _kp_limits("kp_head", K, V, cams.shape[0], verts.shape[0], 1 if kp_gt is None else kp_gt.shape[0])
    _lib.require_gpu(A, verts, cams, kp_gt)
    return _KpHead.apply(A, verts, cams, None if kp_gt is None else kp_gt.detach(), img_size, bool(want_err))


class _CameraLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cam_pred, cam_ref, cams, probs, margin):
        ctx.set_materialize_grads(False)
        p = _f32c(cam_pred)
        r, c, w = [None if t is None else _f32c(t) for t in (cam_ref, cams, probs)]
        N, dev = p.shape[0], p.device
        G = 0 if w is None else w.shape[0]
        loss = torch.empty((), dtype=torch.float32, device=dev)
        best = None if w is None else torch.empty((N,), dtype=torch.int64, device=dev)
        _lib.call("acfm_camera_loss_forward", dev, p, r, c, w, N, G, float(margin), loss, best)
        ctx.save_for_backward(p, r, c, best)
        ctx.margin = float(margin)
        if best is not None:
            ctx.mark_non_differentiable(best)
        return loss, best

    @staticmethod
    def backward(ctx, g, _gb):
        if g is None or not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        p, r, c, best = ctx.saved_tensors
        g = _f32c(g)
        gp = torch.empty_like(p)
        _lib.call("acfm_camera_loss_backward", p.device, p, r, c, best, g, p.shape[0], ctx.margin, gp)
        return gp, None, None, None, None


def camera_loss(cam_pred, cam_ref=None, margin=0., cams=None, probs=None):
    """loss_utils.camera_loss(cam_pred, cam_ref, margin) in one launch each way -> (loss, None); or, with cams [G*N,7]
    and probs [G,N] in place of cam_ref, against the most probable hypothesis of every frame (multiframe/main.py:753-762:
    argmax, gather, detach, camera_loss) -> (loss, best [N] int64 = probs.argmax(0), the smallest g at a tie).
    Only cam_pred receives a gradient."""
    if (cam_ref is None) == (cams is None) or (cams is None) != (probs is None):
        raise ValueError("camera_loss: give either cam_ref [N,7] or cams [G*N,7] with probs [G,N]")
    if cam_pred.dim() != 2 or cam_pred.shape[1] != 7:
        raise ValueError("camera_loss: cam_pred [N,7] expected, got %s" % (tuple(cam_pred.shape),))
    N = cam_pred.shape[0]
    if cam_ref is not None and tuple(cam_ref.shape) != (N, 7):
        raise ValueError("camera_loss: cam_ref [%d,7] expected, got %s" % (N, tuple(cam_ref.shape)))
    if cams is not None and (probs.dim() != 2 or probs.shape[1] != N or probs.shape[0] < 1
                             or tuple(cams.shape) != (probs.shape[0] * N, 7)):
        raise ValueError("camera_loss: cams [G*%d,7] and probs [G,%d] expected, got %s and %s"
                         % (N, N, tuple(cams.shape), tuple(probs.shape)))
    if N > KP_MAX_N:
        raise ValueError("camera_loss: N <= %d cameras, got N = %d" % (KP_MAX_N, N))
    _kp_f32("camera_loss", cam_pred, cam_ref, cams, probs)
    _lib.require_gpu(cam_pred, cam_ref, cams, probs)
    det = lambda t: None if t is None else t.detach()
    return _CameraLoss.apply(cam_pred, det(cam_ref), det(cams), det(probs), margin)
