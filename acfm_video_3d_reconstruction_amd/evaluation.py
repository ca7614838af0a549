"""The numbers of multiframe/benchmark/evaluate.py:132-161, 220-245 (mean IoU, PCK@0.1, PCK@0.15), accumulated on the
tensors' own device with no host read until report()."""
import torch


class BenchStats:
    """stats = BenchStats(img_size, num_kps); stats.update(...) once per batch; stats.report() at the end."""

    def __init__(self, img_size, num_kps):
        self.img_size, self.num_kps = float(img_size), int(num_kps)
        self.ious = []                       # per batch: [B] on the device
        self.n_vis = self.n_pt1 = self.n_pt15 = None

    def update(self, mask_pred, mask_gt, kp_err, kp_vis):
        """mask_pred, mask_gt [B,H,W] (or [B,H*W]); kp_err [B,K] in pixels (ops.kp_head's kp_err, or
        keypoints.pixel_error); kp_vis [B,K], the annotation's visibility column.  evaluate.py:139-146 and the sums of
        :229-233; nothing is read back."""
        B = mask_gt.shape[0]
        gt = mask_gt.reshape(B, -1).to(torch.float32)
        pred = mask_pred.reshape(B, -1).to(torch.float32)
        inter = gt * pred
        union = gt + pred - inter
        self.ious.append(inter.sum(1) / union.sum(1))
        err = kp_err.detach().reshape(B, self.num_kps).to(torch.float32)
        vis = kp_vis.reshape(B, self.num_kps).to(torch.float32)
        sums = [vis.sum(0), ((err < 0.1 * self.img_size) * vis).sum(0), ((err < 0.15 * self.img_size) * vis).sum(0)]
        if self.n_vis is None:
            self.n_vis, self.n_pt1, self.n_pt15 = sums
        else:
            self.n_vis, self.n_pt1, self.n_pt15 = self.n_vis + sums[0], self.n_pt1 + sums[1], self.n_pt15 + sums[2]

    def report(self):
        """evaluate.py:226-243: keypoints never visible are dropped, PCK is the mean of the per-keypoint ratios.
        -> dict(mean_iou, pck1, pck15, n_vis [K] as a host tensor)."""
        if self.n_vis is None:
            raise ValueError("BenchStats.report: no batch was added")
        keep = self.n_vis != 0
        n_vis = self.n_vis[keep]
        return dict(mean_iou=float(torch.cat(self.ious).mean()), pck1=float((self.n_pt1[keep] / n_vis).mean()),
                    pck15=float((self.n_pt15[keep] / n_vis).mean()), n_vis=self.n_vis.cpu())
