"""bench.py's launch contract, on CPU: `--gpus N` started without a launcher spawns N ranks itself (or refuses when fewer than N
GPUs are visible -- never a silent 1-GPU run), and the multi-rank skeleton (rendezvous, barriers, MAX over ranks, ONE JSON line from
rank 0 with n_gpus = N) works over gloo with world_size 2 (`--dry-run`: no device work, marked as not a measurement).  On the GPU:
a plain run measures the headline alone, `--full` everything beside it."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["CUDA_VISIBLE_DEVICES"] = env["HIP_VISIBLE_DEVICES"] = ""
    return env


def test_gpus_n_without_n_gpus_fails_loudly():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "1", "--warmup", "0"], capture_output=True, text=True, env=_env(), timeout=300)
    assert r.returncode != 0
    assert "refusing to run fewer ranks" in r.stderr and not r.stdout.strip()


def test_gpus_2_dry_run_spawns_two_ranks_and_prints_one_line():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "3", "--warmup", "1", "--dry-run"], capture_output=True, text=True,
                       env=_env(), timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    j = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
                "data", "config"):
        assert key in j, key
    assert j["n_gpus"] == 2 and j["steps"] == 3 and j["warmup"] == 1 and j["dry_run"] is True and "NOT a measurement" in j["data"]
    assert j["ms_per_step"] >= 2.0  # rank 1 sleeps 2 ms per step: the MAX over ranks, not rank 0's own 1 ms
    assert j["scaling"] == "weak" and "workload" in j["config"]


def test_mismatched_world_size_is_an_error():
    env = _env()
    env.update(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29512")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--dry-run"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode != 0 and "WORLD_SIZE=1" in (r.stderr + r.stdout)


def test_gpus_8_dry_run_through_the_drivers_launcher():
    """The driver's own command for the 8-GPU line -- `python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1
    --master-port P bench.py --gpus 8 ...` -- on CPU (`--dry-run`, gloo): eight ranks rendezvous, ONE line from rank 0 with n_gpus = 8
    and the MAX over ranks (round-5 verdict item 7: the N = 8 path had never executed in any form)."""
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "8", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), BENCH, "--gpus", "8", "--steps", "2", "--warmup", "1", "--dry-run"],
                       capture_output=True, text=True, env=_env(), timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    j = json.loads(lines[0])
    assert j["n_gpus"] == 8 and j["steps"] == 2 and j["dry_run"] is True and j["scaling"] == "weak"
    assert j["ms_per_step"] >= 8.0  # rank r sleeps (r + 1) ms per step: rank 7's 8 ms is the step, not rank 0's 1 ms


def test_steps_below_one_is_refused():
    r = subprocess.run([sys.executable, BENCH, "--steps", "0", "--dry-run"], capture_output=True, text=True, env=_env(), timeout=300)
    assert r.returncode != 0 and "--steps must be at least 1" in r.stderr and not r.stdout.strip()


def test_dump_outputs_is_refused_where_it_is_not_implemented():
    r = subprocess.run([sys.executable, BENCH, "--workload", "sdxl_attn_int8", "--dump-outputs", "unused"], capture_output=True, text=True,
                       env=_env(), timeout=300)
    assert r.returncode != 0 and "--dump-outputs is not implemented" in r.stderr and not r.stdout.strip()


def test_dump_outputs_writes_float32_within_budget_and_samples_the_same_elements(tmp_path, monkeypatch):
    """bench.dump_outputs on CPU tensors: small outputs whole and exact, large ones a 1-D sample of their own values, the files within
    the byte budget, and the same elements written on every call (two builds are compared output for output)."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES", 400_000)
    g = torch.Generator().manual_seed(0)
    outs = [torch.randn(s, generator=g).to(torch.bfloat16) for s in [(1, 320)] * 3 + [(256, 320)] * 4 + [(1, 8, 16, 16)]]
    layers = [(f"blk{i}.attn/to_q",) for i in range(len(outs))]
    info = [bench.dump_outputs(outs, layers, str(tmp_path / d)) for d in ("a", "b")]
    assert info[0]["arrays"] == len(outs) and 0 < info[0]["sampled_arrays"] < len(outs) and info[0]["bytes"] <= 400_000
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) and len(names) == len(outs) and names[0] == "0000_blk0.attn_to_q.npy"
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) == info[0]["bytes"]
    for i, n in enumerate(names):
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        ref = outs[i].float().numpy()
        assert a.dtype == np.float32 and np.array_equal(a, b)
        if a.shape == ref.shape:
            assert np.array_equal(a, ref)
        else:
            assert a.ndim == 1 and a.size < ref.size and np.isin(a, ref.ravel()).all()


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only_and_full_adds_the_rest():
    """A plain run times the steps and prints the headline; what is measured beside it (roofline, the eager step, cpu_baseline) comes
    with --full only, on the same line (a small slice of the headline's layer list)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    lines = {}
    for mode, extra in (("plain", []), ("full", ["--full", "--cpu-seconds", "0.2"])):
        r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--layers-scale", "0.05"] + extra,
                           capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        out = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(out) == 1, r.stdout
        lines[mode] = json.loads(out[0])
    for j in lines.values():
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "config"):
            assert key in j, key
        assert j["dtype"] == "i8" and j["unit"] == "GOP/s" and j["higher_is_better"] is True and j["value"] > 0 and j["steps"] == 3
    assert lines["plain"]["metric"] == lines["full"]["metric"]
    plain, full = lines["plain"], lines["full"]
    assert not {"roofline", "roofline_error", "cpu_baseline", "cpu_baseline_error"} & set(plain) and "eager_ms_per_step" not in plain["config"]
    assert "roofline" in full and full["roofline"]["launches_per_step"] > 0 and "eager_ms_per_step" in full["config"]
    assert "cpu_baseline" in full and "cfg1" in full["cpu_baseline"]
