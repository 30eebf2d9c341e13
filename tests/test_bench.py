"""bench.py end to end on CPU/gloo: 2 ranks launched through dwamd-run, one
rank SIGKILLed mid-step, the agent restarts from deep standbys, the new
processes restore from shm and finish the fault window.  The JSON line must
report the requested world size and a verified restore."""

import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_two_ranks_real_kill(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--model", "gpt2-tiny", "--micro-batch",
           "2", "--seq", "64", "--steps", "8", "--warmup", "2", "--full", "--fault-window", "16", "--import-window", "12", "--ckpt-dir", str(tmp_path / "ckpt"), "--timeout",
           "240"]
    r = subprocess.run(cmd, env=env, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-20000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    assert res["n_gpus"] == 2 and res["rccl_world"] == 2 and res["config"]["parallelism"] == "dp2"
    assert res["steps"] == 8 and res["warmup"] == 2
    assert res["load_verified"] and res["replicas_identical"]
    assert res["restarts"] == 1 and res["load_verified_after_restart"]
    # the deep standbys formed the restarted world while parked and the
    # restarted workers adopted it (elastic_agent/pg_preform.py)
    assert res["pg_adopted_after_restart"] is True and res["pg_preform_sec"] > 0
    assert res["pg_init_cold_sec"] > 0 and res["recovery_breakdown_s"]["pg_init"] >= 0
    # plumbing check: on CPU a gpt2-tiny step is a few ms and the phase-0 step
    # time it is normalised by is noisy (the value itself is judged on GPUs)
    assert 0 < res["goodput_pct"] < 150
    assert res["lost_steps"] >= 0 and res["recover_sec"] > 0
    assert res["persist_sec"] is not None
    # every timed save produced a checkpoint; skipped saves are reported
    assert res["timed_saves_ok"] is True and res["skipped_saves_timed"] == 0
    assert res["first_save_sec"] is not None and res["skipped_saves_fault_window"] >= 0
    assert "goodput_pct_1fail_per_hour_modelled" in res and "goodput_pct_1fail_per_hour" not in res
    # node-replacement restore from the persisted file, verified against memory
    assert res["load_sec_storage"] > 0 and res["load_storage_verified"] is True
    # the failure again under the default --standby-mode import: cold
    # replacement process, restore from host shm (reference semantics)
    imp = res["import_mode"]
    assert imp["standby_mode"] == "import" and imp["restarts"] == 1 and imp["load_verified_after_restart"]
    assert imp["pg_adopted_after_restart"] is True  # import standbys pre-form too
    assert res["load_sec_shm"] == imp["load_sec"] and res["goodput_pct_import"] == imp["goodput_pct"]
    assert res["recover_sec_import"] > 0 and imp["recovery_breakdown_s"]["process_to_model_built"] is not None
    # and under the framework default (import standbys owning the HBM tier)
    hbm = res["import_mode_hbm"]
    assert hbm["hbm_tier"] is True and hbm["restarts"] == 1 and hbm["load_verified_after_restart"]
    assert res["goodput_pct_import_hbm_tier"] == hbm["goodput_pct"]


def test_bench_plain_run_stops_after_timed_steps(tmp_path):
    """Without --full the run ends after the timed steps: the headline keys
    only, no restart, and --dump-outputs leaves the last step's arrays."""
    import numpy as np

    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    dump = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--model", "gpt2-tiny", "--micro-batch",
           "2", "--seq", "64", "--steps", "5", "--warmup", "1", "--ckpt-dir", str(tmp_path / "ckpt"), "--timeout",
           "120", "--dump-outputs", str(dump)]
    r = subprocess.run(cmd, env=env, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=150)
    assert r.returncode == 0, r.stderr[-20000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    assert res["full"] is False and res["steps"] == 5 and res["warmup"] == 1 and res["n_gpus"] == 1
    assert res["unit"] == "s" and res["higher_is_better"] is False and res["dtype"] == "fp32"
    assert res["value"] == res["save_sec_mean"] > 0 and res["ms_per_step"] > 0
    assert res["timed_saves"] == 2 and res["timed_saves_ok"] is True
    for moved in ("goodput_pct", "load_sec", "restarts", "persist_sec", "time_to_durable_sec", "import_mode", "fsdp"):
        assert moved not in res, moved
    loss = np.load(dump / "loss.npy")
    assert loss.dtype == np.float64 and loss.shape == (5,) and np.isfinite(loss).all()
    assert abs(float(loss[-1]) - res["loss"]) < 1e-3
    assert res["dumped_outputs"] == {"loss": [5]} and sorted(os.listdir(dump)) == ["loss.npy"]
    assert loss[-1] < loss[0]  # the updates between the steps took effect


def test_bench_eight_ranks_sliced(tmp_path):
    """The N=8 path the driver runs on a whole node, rehearsed on CPU/gloo:
    8 ranks, the replicated checkpoint split 8 ways (each rank snapshots and
    restores 1/8; the restore all-gathers), a real SIGKILL and a restart
    from deep standbys."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "8", "--model", "gpt2-tiny", "--micro-batch",
           "1", "--seq", "32", "--steps", "4", "--warmup", "1", "--full", "--fault-window", "12", "--no-import-fault",
           "--no-persist", "--ckpt-dir", str(tmp_path / "ckpt"), "--timeout", "400"]
    r = subprocess.run(cmd, env=env, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=480)
    assert r.returncode == 0, r.stderr[-20000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert res["n_gpus"] == 8 and res["rccl_world"] == 8 and res["config"]["parallelism"] == "dp8"
    assert res["ckpt_slices"] == 8 and res["restore_gather_group"] is True
    assert res["load_verified"] and res["replicas_identical"] and res["timed_saves_ok"]
    assert res["restarts"] == 1 and res["load_verified_after_restart"]
    assert res["pg_adopted_after_restart"] is True  # 8 standbys pre-formed the 8-rank world


def test_framework_rows_plumbing(tmp_path):
    """The FSDP and Megatron-layout flash-checkpoint rows bench.py adds at
    N=1 (tiny models on CPU): both measured, restored and verified."""
    import sys as _sys

    _sys.path.insert(0, REPO)
    import bench

    a = bench.parse(["--model", "gpt2-tiny", "--seq", "64", "--micro-batch", "2", "--ckpt-dir", str(tmp_path / "ck")])
    out = bench.framework_rows(a, str(tmp_path))
    for name in ("fsdp", "megatron"):
        assert name in out, out
        row = out[name]
        assert row["load_verified"] is True and row["save_sec"] > 0 and row["load_sec"] > 0
        assert row["save_vs_baseline"] is None  # ratios only for the reference's GPT2-1.5B
