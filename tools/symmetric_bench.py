"""The symmetric template's mirror + gradient fold (ops.symmetrize, csrc/acfm_deform.hip) against the torch lines of
MeshNet.symmetrize (mesh_net.py:573-591): kernel launches and time of one forward + backward, eager and as a hipGraph
replay, at the level-3 (32, 305) and level-4 (64, 1249) counts; then tools/step_bench.py's step on the level-3 sphere
with and without `symmetric`, each in a fresh process.  usage: python tools/symmetric_bench.py [--no-step]"""
import argparse, os, subprocess, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from acfm_video_3d_reconstruction_amd import ops

p = argparse.ArgumentParser()
p.add_argument("--iters", type=int, default=500); p.add_argument("--repeats", type=int, default=5)
p.add_argument("--no-step", action="store_true"); p.add_argument("--step-iters", type=int, default=20)
a = p.parse_args()
d = torch.device("cuda:0")


def torch_lines(V, n_sym, flip=None):
    if flip is None:              # as the reference writes it: two more launches, and the index write cannot be captured
        flip = torch.ones((1, 3), device=V.device)
        flip[0, 0] = -1
    return torch.cat([V, flip * V[-n_sym:]], 0)


FLIP = torch.tensor([[-1.0, 1.0, 1.0]], device=d)


def launches(fn):
    """Device kernels (and memsets / copies) of one call, counted by torch.profiler."""
    from torch.profiler import profile, ProfilerActivity
    fn(); torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as pr:
        fn(); torch.cuda.synchronize()
    return sum(1 for e in pr.events() if str(e.device_type).endswith("CUDA"))


def timed(fn):
    """Median over repeats of the time per call in a loop of iters calls, microseconds (and the fastest, slowest)."""
    ts = []
    for _ in range(a.repeats):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(a.iters): fn()
        torch.cuda.synchronize(); ts.append(1e6 * (time.perf_counter() - t0) / a.iters)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


for n_indept, n_sym in ((32, 305), (64, 1249)):
    half = torch.randn(n_indept + n_sym, 3, device=d, requires_grad=True)
    w = torch.randn(n_indept + 2 * n_sym, 3, device=d)
    # (f, the same under capture): the reference's `flip[0, 0] = -1` is refused while a stream is capturing, so the
    # captured torch lines get the flip vector built beforehand
    for name, f, fc in (("kernels", lambda: ops.symmetrize(half, n_sym), None),
                        ("torch lines", lambda: torch_lines(half, n_sym), lambda: torch_lines(half, n_sym, FLIP))):
        def one(f=f):
            return torch.autograd.grad(f(), half, w)[0]
        for _ in range(3): one()
        n = launches(one)
        eager = timed(one)
        if fc is not None:
            def one(f=fc):
                return torch.autograd.grad(f(), half, w)[0]
        s = torch.cuda.Stream(); s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2): one()
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = one()
        replay = timed(g.replay)
        print("(%d, %d) %-11s forward + backward: %2d launches, eager %.1f us (%.1f - %.1f), hipGraph replay%s %.1f us "
              "(%.1f - %.1f)" % ((n_indept, n_sym, name, n) + eager + (" (flip prebuilt: %d launches)" % launches(one)
                                                                        if fc is not None else "",) + replay), flush=True)

if not a.no_step:
    for extra in ([], ["--symmetric"], ["--graph"], ["--graph", "--symmetric"]):
        cmd = [sys.executable, os.path.join(ROOT, "tools", "step_bench.py"), "--mesh", "sphere3", "--iters",
               str(a.step_iters)] + extra
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        lines = [l for l in r.stdout.splitlines() if "ms/step" in l]
        print(lines[0] if lines else "step_bench %s failed (exit %d): %s" % (extra, r.returncode, r.stderr[-400:]), flush=True)
        if r.returncode != 0:
            sys.exit(r.returncode)      # (nothing more is started on the device after a failure)
