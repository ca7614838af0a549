#!/usr/bin/env python
"""Times the keypoint + camera-head supervision of the multiframe step, forward + backward, two ways in one process:

  torch:   today's composition exactly as multiframe_step.py writes it with supervision_kernels=False -- softmax, matmul
           over the repeated vertices, ops.project_xy, kp_l2_loss over the repeated ground truth; argmax, gather,
           loss_utils.camera_loss -- and its autograd backward.  Its vertex leaf is the repeated [G*N,V,3] tensor the step
           already holds for its renders.
  kernels: ops.kp_weights + ops.kp_head + ops.camera_loss (csrc/acfm_keypoints.hip), vertices and ground truth unrepeated.

Each shape is warmed up, then the two versions are timed alternately (block by block), synchronised, both eager and as
a hipGraph replay; a torch.profiler pass of its own counts the kernel launches of one forward + backward of each.
One JSON line per shape with the timings, then one with the launch counts.  Needs the GPU: there is no CPU fallback.

    python tools/keypoint_bench.py --reps 200 --warmup 20 [--out FILE]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from acfm_video_3d_reconstruction_amd import ops                                     # noqa: E402
from acfm_video_3d_reconstruction_amd.nnutils import loss_utils                      # noqa: E402

SHAPES = [(frames, G, K, V) for frames, G in ((32, 3), (64, 1)) for K in (15, 19) for V in (642, 2562)]
KP_WT, CAM_WT = 1.0, 2.0


def make_inputs(frames, G, K, V, device, seed=0):
    g = torch.Generator().manual_seed(seed)
    N = frames
    cams = torch.randn(G * N, 7, generator=g)
    cams[:, 0], cams[:, 1:3] = 0.8, cams[:, 1:3] * 0.05
    cams[:, 3:] = torch.nn.functional.normalize(cams[:, 3:], dim=1)
    t = dict(vert2kp=3 * torch.randn(K, V, generator=g), pred_v1=0.5 * torch.randn(N, V, 3, generator=g), cam=cams,
             kps=torch.cat([0.5 * torch.randn(N, K, 2, generator=g), (torch.rand(N, K, 1, generator=g) > 0.3).float()], 2),
             probs=torch.softmax(torch.randn(G, N, generator=g), 0), pc=torch.randn(N, 7, generator=g))
    t = {k: v.to(device) for k, v in t.items()}
    t["pred_v"] = t["pred_v1"].repeat(G, 1, 1)
    for k in ("vert2kp", "pred_v1", "pred_v", "cam", "pc"):
        t[k].requires_grad_(True)
    return t


def torch_version(t, G, N):
    kp_v = torch.matmul(torch.softmax(t["vert2kp"], dim=1), t["pred_v"])
    kp = loss_utils.kp_l2_loss(ops.project_xy(kp_v, t["cam"], 0.), t["kps"].repeat(G, 1, 1), reduction="none")
    best = t["probs"].reshape(G, N).argmax(dim=0)
    cam_sel = t["cam"].reshape(G, N, 7)[best, torch.arange(N, device=t["cam"].device)]
    cam_head = loss_utils.camera_loss(t["pc"], cam_sel.detach(), 0)
    total = KP_WT * (kp.reshape(G, N) * t["probs"]).sum(0).mean() + CAM_WT * cam_head
    # (total is returned detached: a live autograd graph would carry its leaves' accumulation nodes, and the stream they
    # were made on, into the next capture)
    return (total.detach(),) + torch.autograd.grad(total, (t["vert2kp"], t["pred_v"], t["cam"], t["pc"]))


def kernel_version(t, G, N):
    A, _ = ops.kp_weights(t["vert2kp"])
    kp = ops.kp_head(A, t["pred_v1"], t["cam"], t["kps"])[2]
    cam_head, _ = ops.camera_loss(t["pc"], cams=t["cam"], probs=t["probs"])
    total = KP_WT * (kp.reshape(G, N) * t["probs"]).sum(0).mean() + CAM_WT * cam_head
    return (total.detach(),) + torch.autograd.grad(total, (t["vert2kp"], t["pred_v1"], t["cam"], t["pc"]))


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e6


def capture(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = fn()
    return graph, outs


def count_launches(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return sum(1 for n in names if "memcpy" not in n.lower() and "memset" not in n.lower())


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=5, help="alternations of the two versions; the median block is reported")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("keypoint_bench: needs the GPU (there is no CPU fallback)")
    d = torch.device("cuda:0")
    lines = []
    for frames, G, K, V in SHAPES:
        t, t2 = make_inputs(frames, G, K, V, d), make_inputs(frames, G, K, V, d)     # the same values, leaves of their own
        fns = {"torch": lambda: torch_version(t, G, frames), "kernels": lambda: kernel_version(t2, G, frames)}
        ref, got = fns["torch"](), fns["kernels"]()
        gv_ref = ref[2].reshape(G, frames, V, 3).sum(0)                          # what the repeat's backward would form
        diffs = [float((got[0] - ref[0]).abs()), float((got[1] - ref[1]).abs().max() / ref[1].abs().max()),
                 float((got[2] - gv_ref).abs().max() / gv_ref.abs().max()),
                 float((got[3] - ref[3]).abs().max() / ref[3].abs().max()),
                 float((got[4] - ref[4]).abs().max() / ref[4].abs().max())]
        graphs = {k: capture(f) for k, f in fns.items()}
        replays = {k: g[0].replay for k, g in graphs.items()}
        for f in list(fns.values()) + list(replays.values()):
            timed(f, args.warmup)
        res = {"eager": {k: [] for k in fns}, "graph": {k: [] for k in fns}}
        for _ in range(args.blocks):
            for k in fns:
                res["eager"][k].append(timed(fns[k], args.reps))
            for k in fns:
                res["graph"][k].append(timed(replays[k], args.reps))
        med = lambda xs: sorted(xs)[len(xs) // 2]
        line = dict(frames=frames, G=G, K=K, V=V, reps=args.reps, blocks=args.blocks,
                    eager_us={k: round(med(v), 2) for k, v in res["eager"].items()},
                    graph_us={k: round(med(v), 2) for k, v in res["graph"].items()},
                    graph_us_min_max={k: [round(min(v), 2), round(max(v), 2)] for k, v in res["graph"].items()},
                    kernels_vs_torch=dict(zip(("total_abs", "d_vert2kp", "d_verts", "d_cams", "d_predicted_camera"), diffs)))
        print(json.dumps(line), flush=True)
        lines.append(line)
        del graphs, replays
    # the launch counts: a profiler pass of its own, after every timing (tracing slows the host)
    for line in lines:
        frames, G, K, V = line["frames"], line["G"], line["K"], line["V"]
        t = make_inputs(frames, G, K, V, d)
        launches = {"torch": count_launches(lambda: torch_version(t, G, frames)),
                    "kernels": count_launches(lambda: kernel_version(t, G, frames))}
        line["launches"] = launches
        print(json.dumps(dict(frames=frames, G=G, K=K, V=V, launches=launches)), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
