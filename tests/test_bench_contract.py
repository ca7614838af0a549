"""The committed bench line (profiles/rNN_bench.json) carries every field the benchmark contract
names; bench.py parses, and its options and output dump behave (CPU: no GPU needed).  The two tests
marked gpu run a small plain and a small --full benchmark in a child process."""
import ast
import glob
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_py_parses_and_defaults_finish_quickly():
    src = open(os.path.join(ROOT, "bench.py")).read()
    ast.parse(src)
    assert '"--gpus", type=int, default=1' in src
    assert '"--steps", type=int, default=30' in src and '"--warmup", type=int, default=10' in src


def test_committed_bench_lines_follow_the_contract():
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_bench.json")))
    assert files, "no committed bench line under profiles/"
    base = json.load(open(os.path.join(ROOT, "BASELINE.json")))
    for fn in files:
        j = json.loads(open(fn).read().strip().splitlines()[-1])
        for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                  "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
            assert k in j, (fn, k)
        assert j["unit"] == "frames/s" and j["higher_is_better"] is True and j["scaling"] == "weak"
        assert j["vs_baseline"] is None and not base.get("published")      # no published number for this metric
        assert j["data"] == "synthetic" and "workload" in j["config"] and "model" not in j["config"]
        assert abs(j["value"] - j["n_gpus"] * j["config"]["frames_per_gpu"] / (j["ms_per_step"] * 1e-3)) < 0.01 * j["value"]
        r = j["roofline"]
        assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s")
        assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
        assert abs(r["achieved"] - r["algorithmic_bytes_per_launch"] / (r["avg_launch_us"] * 1e-6) / 1e9) < 0.01 * r["achieved"]
        c = j["cpu_baseline"]
        assert c["kind"] in ("port", "reference") and c["cores"] >= 1 and c["value"] > 0 and c["sample"]


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_plain_run_is_the_default_and_full_dump_are_options(monkeypatch):
    import sys
    b = _bench_module()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = b.parse()
    assert (a.gpus, a.steps, a.warmup, a.full, a.dump_outputs) == (1, 7, 2, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "outs"])
    a = b.parse()
    assert a.full is True and a.dump_outputs == "outs"


def test_dump_outputs_dtypes_and_size_cap(tmp_path):
    import numpy as np
    import torch
    b = _bench_module()
    big = torch.arange(3 * 10**6, dtype=torch.float32)
    named = dict(loss=torch.tensor(1.5), g64=torch.ones(4, 3, dtype=torch.float64), g16=torch.ones(5, dtype=torch.float16),
                 big=big, unused=None)
    assert b.dump_outputs(str(tmp_path / "all"), named) == ["big", "g16", "g64", "loss"]
    got = {n: np.load(str(tmp_path / "all" / (n + ".npy"))) for n in ("big", "g16", "g64", "loss")}
    assert got["loss"].dtype == np.float32 and got["loss"].shape == () and got["loss"] == 1.5
    assert got["g64"].dtype == np.float64 and got["g64"].shape == (4, 3)
    assert got["g16"].dtype == np.float32
    np.testing.assert_array_equal(got["big"], big.numpy())
    # over the cap: the small arrays whole, the big one a sorted sample of its elements, the same in every run
    limit = 10**6
    for d in ("cut1", "cut2"):
        b.dump_outputs(str(tmp_path / d), named, limit=limit)
    files = sorted(os.listdir(str(tmp_path / "cut1")))
    assert sum(os.path.getsize(str(tmp_path / "cut1" / f)) for f in files) <= limit
    s1, s2 = (np.load(str(tmp_path / d / "big.npy")) for d in ("cut1", "cut2"))
    assert s1.ndim == 1 and 0 < s1.size < big.numel() and np.all(np.diff(s1) > 0)
    np.testing.assert_array_equal(s1, s2)
    np.testing.assert_array_equal(np.load(str(tmp_path / "cut1" / "g64.npy")), got["g64"])


def _run_bench(args, timeout):
    import subprocess
    import sys
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["bench.py"] + args
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_bench_run_times_the_steps_and_dumps_outputs(tmp_path):
    import numpy as np
    small = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--frames", "4", "--img", "64"]
    j = _run_bench(small + ["--dump-outputs", str(tmp_path / "a")], 600)
    assert j["steps"] == 3 and j["warmup"] == 1 and j["full"] is False
    assert j["unit"] == "frames/s" and j["higher_is_better"] is True and j["dtype"] == "f32"
    assert abs(j["value"] - 4 / (j["ms_per_step"] * 1e-3)) < 0.01 * j["value"]
    assert j["roofline"] is None and j["cpu_baseline"] is None and j["kernels"] is None
    assert "render_only" not in j and "eager_launch" not in j
    names = sorted(os.listdir(str(tmp_path / "a")))
    assert names == ["grad_atlas.npy", "grad_cams.npy", "grad_delta.npy", "grad_mean.npy", "loss.npy"]
    g = {n[:-4]: np.load(str(tmp_path / "a" / n)) for n in names}
    assert g["grad_delta"].shape == (4, 16, 3) and g["grad_cams"].shape == (4, 7) and g["grad_atlas"].shape[0] == 4
    assert all(np.isfinite(v).all() and v.dtype == np.float32 for v in g.values())
    assert np.abs(g["grad_cams"]).max() > 0


@pytest.mark.gpu
def test_full_bench_run_fills_every_field():
    j = _run_bench(["--gpus", "1", "--steps", "2", "--warmup", "2", "--frames", "4", "--img", "64", "--cpu-seconds", "0.5", "--full"], 600)
    assert j["full"] is True and j["steps"] == 2
    assert j["kernels"] and j["roofline"]["kernel"] in j["kernels"]
    assert j["cpu_baseline"]["value"] > 0 and j["gpu_over_cpu"] > 0
    for leg in ("eager_launch", "shared_shape_step", "all_slots_stored", "fused_render_loss", "deterministic_backward",
                "reference_call_sequence", "render_only", "survey_8d_step"):
        assert j[leg]["ms_per_step"] > 0, leg
