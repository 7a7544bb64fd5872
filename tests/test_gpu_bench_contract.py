"""bench.py and __graft_entry__.smoke() are the driver's entry points: run them as the driver does and check the JSON contract."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent

REQUIRED = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
            "data", "config", "roofline", "cpu_baseline"}


def _run(args, env=None):
    r = subprocess.run([sys.executable, str(ROOT / "bench.py")] + args, capture_output=True, text=True, timeout=600, cwd=str(ROOT),
                       env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.strip().splitlines() if l.strip()]
    return json.loads(lines[-1])            # the record is the LAST stdout line


def test_bench_json_contract_default_workload():
    out = _run(["--gpus", "1", "--steps", "256", "--warmup", "32", "--full"], env={"USIM_CPU_BUDGET_S": "2"})
    assert REQUIRED <= set(out)
    assert out["metric"].startswith("env-steps/sec") and out["unit"] == "env-steps/s" and out["higher_is_better"] is True
    assert out["n_gpus"] == 1 and out["steps"] == 256 and out["warmup"] == 32 and out["scaling"] == "weak" and out["vs_baseline"] is None
    assert out["dtype"] == "f32" and out["data"] == "synthetic" and "workload" in out["config"] and "model" not in out["config"]
    assert out["config"]["presteps"] == 0              # no untimed steps besides the W warm-up steps (bench.py --presteps is for studies)
    assert out["value"] > 1e6 and abs(out["value"] - 4096 * 256 / (out["ms_per_step"] * 256e-3)) / out["value"] < 1e-6
    rf = out["roofline"]
    assert rf["bound"] in ("hbm", "mfma") and rf["unit"] == "GB/s" and rf["peak"] == 8000.0
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-12 and rf["achieved"] > 0
    assert rf["algorithmic_bytes_per_env_step"] == 1912 and (rf["traffic"] is None or rf["traffic"] > 1e5)
    assert rf["algorithmic_bytes_per_launch"] == 1912 * 4096 * rf["steps_per_launch"] and 1 <= rf["steps_per_launch"] <= 256
    assert abs(rf["avg_launch_us"] - rf["avg_kernel_us"] * rf["steps_per_launch"]) < 1e-6 * rf["avg_launch_us"]
    assert abs(rf["achieved"] - rf["algorithmic_bytes_per_launch"] / rf["avg_launch_us"] * 1e-3) < 1e-6 * rf["achieved"]
    assert out["ranks_seen"] == 1 and out["gather"] is None and out["config"]["domain_randomisation"] == "stiffness+damping"
    iss = rf["issue"]                                      # measured issue figures of the committed PMC profile (profiles/<round>/issue.json), not a flop guess
    assert iss is None or (1e3 < iss["valu_inst_per_wave_step"] < 1e4 and 0 < iss["valu_active_share_of_wave_cycles"] < 1)
    assert (iss is None) == (rf["issue_source_config"] is None)          # a quoted profile figure names the command it was measured on
    assert "valu_frac" not in rf
    cb = out["cpu_baseline"]
    assert cb["kind"] == "port" and cb["unit"] == "env-steps/s" and cb["value"] > 0 and cb["cores"] >= 1 and "sample" in cb


def test_bench_plain_run_is_lean_and_dumps_the_last_step(tmp_path):
    """without --full: the headline line and nothing that takes runs of its own; --dump-outputs writes the last timed step's rows of the rollout
    block, and the same arguments give the same outputs"""
    import numpy as np
    dumps = []
    for k in range(2):
        d = tmp_path / f"run{k}"
        out = _run(["--gpus", "1", "--steps", "64", "--warmup", "16", "--dump-outputs", str(d)])
        assert REQUIRED - {"cpu_baseline"} <= set(out) and "cpu_baseline" not in out
        assert out["steps"] == 64 and out["ms_per_step"] > 0 and abs(out["value"] - 4096 / (out["ms_per_step"] * 1e-3)) / out["value"] < 1e-6
        dumps.append({p.stem: np.load(p) for p in d.iterdir()})
    a, b = dumps
    assert set(a) == {"obs", "act", "rew", "done"} and all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
    assert a["obs"].shape == (4096, 19) and a["act"].shape[0] == 4096 and a["rew"].shape == (4096,) and a["done"].shape == (4096,)
    assert set(np.unique(a["done"])) <= {0.0, 1.0} and np.abs(a["obs"]).max() > 0
    assert all(np.array_equal(a[k], b[k]) for k in a)


def test_bench_gather_path_over_rccl_with_one_rank():
    """configs[3] cannot run here (one GPU per box), but its code path can: the process group over backend "nccl" (= RCCL), the all-gather of every rollout block on
    the side stream while the next block is simulated, the per-rank record -- everything `bench.py --gpus N` does, with a world of one"""
    out = _run(["--steps", "512", "--warmup", "32", "--block", "128", "--no-cpu-baseline"], env={"USIM_BENCH_FORCE_GATHER": "1"})
    g = out["gather"]
    assert out["ranks_seen"] == 1 and g["kind"] == "rccl" and g["backend"] == "nccl" and g["blocks_in_timed_region"] == 4
    assert g["result_shape"] == [1, 128, 4096, 19 + 6 + 2] and g["last_ms"] is not None and g["last_ms"] > 0 and g["block_ms"] > 0
    assert isinstance(g["hidden_behind_next_block"], bool)
    pr = out["per_rank"]
    assert len(pr["avg_kernel_us"]) == 1 and 5 < pr["avg_kernel_us"][0] < 60 and pr["gather_last_ms"][0] == pytest.approx(g["last_ms"])
    assert "RCCL all-gather" in out["config"]["parallelism"] and out["value"] > 5e7


def test_bench_rigid_workload_and_block_tail():
    out = _run(["--steps", "200", "--warmup", "10", "--workload", "rigid", "--no-cpu-baseline", "--block", "64"])
    assert out["roofline"]["algorithmic_bytes_per_env_step"] == 316 and "cpu_baseline" not in out and out["value"] > 1e7


def test_bench_full_torso_workload():
    """`bench.py --workload full`: the full torso (csrc/usim_full.h) through the same contract -- its own algorithmic bytes (4752), one step per launch"""
    out = _run(["--steps", "12", "--warmup", "4", "--workload", "full", "--envs-per-gpu", "512", "--no-cpu-baseline"])
    assert out["roofline"]["algorithmic_bytes_per_env_step"] == 4752 and out["config"]["steps_per_launch"] == 1 and out["config"]["lanes_per_env"] == 64
    assert "FULL torso" in out["config"]["workload"] and out["value"] > 1e5 and out["roofline"]["frac"] < 0.01


def test_graft_entry_smoke():
    r = subprocess.run([sys.executable, str(ROOT / "__graft_entry__.py"), "smoke"], capture_output=True, text=True, timeout=600, cwd=str(ROOT))
    assert r.returncode == 0 and "smoke ok" in r.stdout, r.stdout + r.stderr
