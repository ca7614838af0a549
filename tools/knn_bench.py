"""Timing and peak memory of ops.knn_points at the template fit's size (5000 x 5000 points), forward and forward +
backward, for N in {1, 8} and K in {1, 8, 32}.  The comparison is the torch composition on the same device: explicit
squared distances ([N,P1,P2]) + topk(largest=False), the distances to the chosen points recomputed for the backward.
At K = 1 one direction of ops.chamfer_nearest is timed as well (it always searches both directions: its time is
halved, and said so).  Events around every call, warm-up, median; peak memory above the inputs.
Every (N, K) runs in a child process of its own under a time limit; the first one that fails ends the run.
usage: python tools/knn_bench.py [--reps 50] [--points 5000] [--limit 120]"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--points", type=int, default=5000)
ap.add_argument("--limit", type=int, default=120, help="seconds per (N, K) child process")
ap.add_argument("--one", type=int, nargs=2, metavar=("N", "K"), help="(internal) measure this pair in this process")
a = ap.parse_args()

if a.one is None:
    print("| N | K | knn fwd us | torch fwd us | knn fwd+bwd us | torch fwd+bwd us | knn peak MB | torch peak MB | chamfer_nearest / 2 us |")
    print("|---|---|---|---|---|---|---|---|---|")
    sys.stdout.flush()
    for N in (1, 8):
        for K in (1, 8, 32):
            cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--warmup", str(a.warmup),
                   "--points", str(a.points), "--one", str(N), str(K)]
            try:
                rc = subprocess.run(cmd, timeout=a.limit).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                sys.exit("N = %d K = %d ended with status %d: stopping" % (N, K, rc))
    sys.exit(0)

sys.path.insert(0, ROOT)
import torch  # noqa: E402

from acfm_video_3d_reconstruction_amd import ops  # noqa: E402

N, K = a.one
P = a.points
d = torch.device("cuda:0")
torch.manual_seed(0)
p1 = (torch.rand(N, P, 3, device=d) * 2 - 1).requires_grad_(True)
p2 = (torch.rand(N, P, 3, device=d) * 2 - 1).requires_grad_(True)
g = torch.rand(N, P, K, device=d)


def knn_fwd():
    return ops.knn_points(p1.detach(), p2.detach(), K=K)


def knn_both():
    return torch.autograd.grad(ops.knn_points(p1, p2, K=K)[0], [p1, p2], g)


def _torch_knn(a1, a2):
    with torch.no_grad():
        e = a1[:, :, None, :] - a2[:, None, :, :]
        d2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
        dist, idx = d2.topk(K, dim=2, largest=False)
    return dist, idx


def torch_fwd():
    return _torch_knn(p1.detach(), p2.detach())


def torch_both():
    _, idx = _torch_knn(p1, p2)
    near = p2[:, :, None, :].expand(N, P, K, 3).gather(1, idx[..., None].expand(N, P, K, 3))
    e = p1[:, :, None, :] - near
    return torch.autograd.grad((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2], [p1, p2], g)


def chamfer():
    return ops.chamfer_nearest(p1.detach(), p2.detach())


def median_us(fn):
    for _ in range(a.warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)]
    for e0, e1 in ev:
        e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return sorted(e0.elapsed_time(e1) for e0, e1 in ev)[a.reps // 2] * 1e3


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(d)
    before = torch.cuda.memory_allocated(d)
    out = fn()
    torch.cuda.synchronize()
    del out
    return (torch.cuda.max_memory_allocated(d) - before) / 2 ** 20


dk, ik = knn_fwd()
dt, it = torch_fwd()
same = float((ik == it).float().mean())        # (topk does not promise the lowest index among equal distances)
assert same > 0.999 and float((dk - dt).abs().max()) <= 1e-6 * float(dt.abs().max()), same
row = [median_us(knn_fwd), median_us(torch_fwd), median_us(knn_both), median_us(torch_both), peak_mb(knn_both), peak_mb(torch_both)]
tail = "%.1f" % (median_us(chamfer) / 2.0) if K == 1 else "-"
print("| %d | %d | %.1f | %.1f | %.1f | %.1f | %.2f | %.2f | %s |" % (N, K, *row, tail))
