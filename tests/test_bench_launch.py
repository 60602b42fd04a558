"""bench.py launch contract: `python bench.py --gpus N` with N > 1 outside torchrun either launches N ranks
itself (fresh `torch.distributed.run` child, before any GPU call) or exits non-zero — it never prints a line for fewer ranks."""
import json
import math
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}


def _json_line(out):
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out[-2000:]
    return json.loads(lines[0])


def test_self_launch_starts_n_ranks_on_cpu():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--launch-check", "--backend", "gloo", "--single-device"],
                       env=ENV, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    line = _json_line(p.stdout)
    assert line["n_gpus"] == 2 and line["ranks_sum"] == 3.0 and line["backend"] == "gloo"
    assert "launching 2 ranks" in p.stderr


def test_more_ranks_than_gpus_exits_nonzero_without_a_line():
    import torch
    n = torch.cuda.device_count() + 1
    if n < 2:
        n = 2
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(max(n, 9))], env=ENV, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode != 0 and not [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert "refusing" in p.stderr


def test_world_size_mismatch_exits_nonzero():
    env = dict(ENV, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--launch-check"], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 2 and "does not match WORLD_SIZE" in p.stderr and not p.stdout.strip()


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _padded_arena(shapes, align):
    """Stand-in for desta.optim.ParamArena: true element k holds k (params) / -k (grads), the alignment padding holds NaN."""
    import math
    import types
    import torch
    a = types.SimpleNamespace(names=[], shapes={}, offsets={})
    off = 0
    for i, s in enumerate(shapes):
        a.names.append(f"t{i}")
        a.shapes[f"t{i}"], a.offsets[f"t{i}"] = tuple(s), off
        off += -(-math.prod(s) // align) * align
    a.params, a.grads = torch.full((off,), float("nan")), torch.full((off,), float("nan"))
    k = 0
    for n in a.names:
        m, o = math.prod(a.shapes[n]), a.offsets[n]
        a.params[o:o + m] = torch.arange(k, k + m, dtype=torch.float32)
        a.grads[o:o + m] = -a.params[o:o + m]
        k += m
    return a


def test_dump_outputs_samples_true_elements_only(tmp_path):
    """--dump-outputs: float32 files, every true element when the arena is small, otherwise a fixed seeded sample that never
    lands on alignment padding and does not depend on the padding."""
    import numpy as np
    import torch
    bench = _bench_module()
    shapes = [(3, 5), (7,), (100, 33), (1,), (50, 50)]
    n_true = 15 + 7 + 3300 + 1 + 2500
    for max_elems in (1 << 22, 500):
        got = []
        for align in (64, 256):
            d = tmp_path / f"{max_elems}_{align}"
            bench.dump_outputs(str(d), torch.tensor(1.25), _padded_arena(shapes, align), max_elems=max_elems)
            f = {k: np.load(d / f"{k}.npy") for k in ("loss", "params", "grads")}
            assert all(v.dtype == np.float32 for v in f.values()) and f["loss"].tolist() == [1.25]
            assert f["params"].size == min(n_true, max_elems) and np.isfinite(f["params"]).all()
            assert (f["grads"] == -f["params"]).all()
            got.append(f["params"])
        assert (got[0] == got[1]).all()
        if max_elems > n_true:
            assert (got[0] == np.arange(n_true)).all()


@pytest.mark.gpu
def test_two_rank_bench_on_one_card_reports_the_exchange(tmp_path):
    """The real bench through its own launcher at N = 2 (two ranks share cuda:0 over gloo: the box has one GPU): n_gpus == 2,
    the all-reduce / wait_update fields are present, value = steps / time (optimizer steps of the node), gpu_batch_steps_per_s = 2 x that."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--single-device",
                        "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-kernel-pass", "--no-calibration", "--dump-outputs", str(tmp_path)],
                       env=dict(ENV, HSA_ENABLE_IPC_MODE_LEGACY="0"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=1500)
    assert p.returncode == 0, p.stderr[-3000:]
    line = _json_line(p.stdout)
    assert line["n_gpus"] == 2 and line["config"]["parallelism"] == "dp2" and line["config"]["global_batch"] == 16
    assert line["bytes_allreduced"] > 5e8 and line["allreduce_ms"] > 0 and line["wait_update_stall_ms"] >= 0
    assert line["comm_backend"] == "gloo"
    # value = OPTIMIZER steps per second of the node (global batch 8 x N per step); the per-GPU aggregates sit beside it
    per_s = 1.0 / (line["ms_per_step"] * 1e-3)
    assert abs(line["value"] - per_s) < 1e-6 and abs(line["gpu_batch_steps_per_s"] - 2 * per_s) < 1e-6
    assert abs(line["samples_per_s"] - 16 * per_s) < 1e-5
    assert line["steps"] == 2 and len(line["ms_per_step_each"]) == 2
    import numpy as np
    loss, params, grads = (np.load(tmp_path / f"{k}.npy") for k in ("loss", "params", "grads"))
    assert abs(float(loss[0]) - line["final_loss"]) < 1e-6 * max(1.0, abs(line["final_loss"]))
    assert params.shape == grads.shape == (1 << 22,) and np.isfinite(params).all() and np.isfinite(grads).all()
    assert np.count_nonzero(grads) > 0.9 * grads.size


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only_and_full_adds_the_legs():
    """A plain run times the steps and prints their line without the legs that take work of their own; --full (CPU baselines
    left out here: minutes on the host) adds the box calibration, the un-overlapped kernel pass and the reference point."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1"]
    lines = {}
    for name, extra in (("plain", []), ("full", ["--full", "--no-cpu-baseline"])):
        p = subprocess.run(cmd + extra, env=ENV, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
        assert p.returncode == 0, p.stderr[-3000:]
        lines[name] = _json_line(p.stdout)
    for line in lines.values():
        assert line["unit"] == "steps/s" and line["higher_is_better"] is True and line["dtype"] == "bf16"
        assert line["steps"] == 2 and line["warmup"] == 1 and len(line["ms_per_step_each"]) == 2
        assert abs(line["value"] - 1e3 / line["ms_per_step"]) < 1e-6 and math.isfinite(line["final_loss"])
    plain, full = lines["plain"], lines["full"]
    assert plain["metric"] == full["metric"] and plain["final_loss"] == full["final_loss"]      # the same steps, legs outside them
    assert not {"box_calibration", "roofline", "pytorch_rocm_reference_point", "cpu_baseline"} & set(plain)
    assert full["box_calibration"]["gemm_gate_up_tflops"] > 0 and full["pytorch_rocm_reference_point"]["speedup_of_this_run"] > 0
    assert full["roofline"]["achieved"] > 0 and full["roofline"]["launches_per_step"] > 0 and full["roofline"]["hbm_kernels"]
    assert "cpu_baseline" not in full
