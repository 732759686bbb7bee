"""bench.py as the driver runs it: plain ``python bench.py --gpus N ...`` (N > 1 starts its own ranks), one JSON line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SA_EPOCHS = 60
SA_ERR_BOUNDS = (0.075, 0.07, 0.11)  # per predicted window: 3x profiles/r03_sa_fixed_epochs.txt (0.0246, 0.0225, 0.0370)
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*flags, timeout=900, extra_env=None, expect_rc=0):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "SAA_BENCH_T0"):
        env.pop(k, None)
    env.update(extra_env or {})
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), *flags], capture_output=True, text=True,
                       timeout=timeout, env=env, cwd=REPO)
    if expect_rc == 0:
        assert r.returncode == 0, r.stderr[-3000:]
    else:
        assert r.returncode != 0, r.stdout[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, (r.stdout[-2000:], r.stderr[-2000:])
    return json.loads(lines[0])


def test_two_ranks_launch_themselves_and_print_one_line():
    """N = 2 on the one-GPU box: both ranks share cuda:0, gloo process group (what --same-device is for)."""
    out = _run("--gpus", "2", "--same-device", "--backend", "gloo", "--refine", "4", "--steps", "40", "--warmup", "10",
               "--sa-train-epochs", str(SA_EPOCHS), "--sa-truth-steps", "24000", "--min-timed-ms", "50", "--full")
    assert out["n_gpus"] == 2 and out["steps"] == 40 and out["warmup"] == 10 and out["timed_calls"] >= 1
    assert out["metric"] == "element_updates_per_s" and out["value"] > 0 and out["scaling"] == "weak"
    assert "2 x-slab" in out["config"]["workload"]
    assert abs(out["value"] - 150 * 4 ** 3 * 1e3 / out["ms_per_step"]) < 1e-6 * out["value"]
    # configs[4]: models trained in the run on the synchronised history, accuracy reported per window
    sa = out["sync_avoiding"]
    assert sa["value"] > 0 and sa["state_finite"] and sa["steps"] == 3 * 3000
    # A FIXED number of epochs with fixed seeds (the time bound is only a cap): what the model is does not depend on how
    # busy the box is.  The bounds are 3x what this very configuration gave on MI355X (profiles/r03_sa_fixed_epochs.txt);
    # what is left to vary is fp32 summation order inside MIOpen.
    tr = sa["training"]
    assert tr["epochs"] == tr["epochs_min_over_ranks"] == SA_EPOCHS and tr["schedule"] == "fixed epoch count", tr
    assert tr["train_mse_first_last"][1] < 0.05 * tr["train_mse_first_last"][0], tr
    errs = sa["rel_l2_vs_synchronised"]
    assert len(errs) == 3 and all(0 <= e < b for e, b in zip(errs, SA_ERR_BOUNDS)), (errs, SA_ERR_BOUNDS)
    assert out["legs"]["headline"] == "done" and out["legs"]["sync_avoiding"] == "done", out["legs"]
    assert out["leg_seconds"]["total"] < out["budget_s"]


def test_line_survives_a_hung_preflight_and_a_stalled_rccl_leg():
    """The 8-GPU record must never be lost to a leg that misbehaves: with the preflight child hanging
    and the RCCL leg stalled for good, the run still prints its one line - headline and sync-avoiding leg measured, the
    failed legs marked - inside its budget, and leaves with a non-zero status so that the hang is seen."""
    import time

    t0 = time.time()
    out = _run("--gpus", "2", "--same-device", "--backend", "gloo", "--refine", "4", "--steps", "40", "--warmup", "10",
               "--sa-train-epochs", "3", "--sa-truth-steps", "12000", "--budget-s", "240", "--force-preflight",
               "--force-rccl-leg", "--min-timed-ms", "50", "--preflight-limit-s", "20", "--rccl-leg-limit-s", "25",
               "--full", expect_rc=3,
               extra_env={"SAA_BENCH_HOOKS": "tests.bench_hooks", "SAA_BENCH_HOOK_PLAN": "preflight=hang,rccl_leg=hang"})
    wall = time.time() - t0
    assert wall < 240, wall
    assert out["value"] > 0 and out["config"]["peer_preflight_rank0"] is False
    assert "all-reduce" in out["config"]["exchange"]  # the fall-back transport carried the headline
    legs = out["legs"]
    assert legs["preflight"].startswith("failed or exceeded") and out["leg_seconds"]["preflight"] <= 22
    assert legs["headline"] == "done" and legs["sync_avoiding"] == "done" and out["sync_avoiding"]["value"] > 0
    assert legs["rccl_allreduce"].startswith("unfinished") and out["rccl_allreduce"]["value"] is None
    assert out["leg_seconds"]["total"] <= 150  # (far inside the budget: the legs' own limits cut the hangs off)


def test_headline_at_the_drivers_flags_is_warm():
    """The driver's own command (BENCH_r01.json: --steps 20 --warmup 5).  Round 1 timed a cold first cooperative
    launch there (33x below the kernel's rate); the timed call must run warm and agree with the kernel-level figure."""
    out = _run("--gpus", "1", "--steps", "20", "--warmup", "5", "--no-cpu-baseline", "--min-timed-ms", "200",
               "--legs", "roofline,per_gpu_of_8,cache_exceeding,predictor", "--big-refine", "10", "--full")
    roof = out["roofline"]
    assert roof["launches_timed"] >= 10 and 0.3 < roof["frac"] < 1.5
    assert roof["timed_region_ms"] >= 900 and roof["short_region"]["launches"] == 12   # sustained figure beside the short one
    # counters from committed profiles are printed only for the plan that was profiled - and then name the limiter
    if roof["traffic"] is not None:
        assert roof["hbm_measured"]["traffic_over_algorithmic"] < 1.0 and roof["bound"].startswith("on-chip"), roof["bound"]
    # the per-GPU workload of configs[3] / [4] (here on a small beam) through every route a step can take
    per = out["per_gpu_of_8"]
    assert out["legs"]["per_gpu_of_8"] == "done", (out["legs"], per)
    assert set(per["routes"]) == {"plain", "peer_loopback", "rccl_eager", "rccl_graph", "sync_avoiding"}
    assert all(r["us_per_step"] > 0 for r in per["routes"].values()) and per["routes"]["sync_avoiding"]["state_finite"]
    assert per["routes"]["sync_avoiding"]["windows"] >= 3 and set(per["projected_8gpu"]["element_updates_per_s"]) == \
        {"peer_loopback", "rccl_eager", "rccl_graph", "sync_avoiding"}
    big = out["cache_exceeding"]
    assert out["legs"]["cache_exceeding"] == "done" and big["ms_per_step"] > 0 and 0 < big["roofline"]["frac"] < 1.5, big
    assert out["legs"]["unstructured"].startswith("skipped")
    # the practical HBM ceiling comes from the library's own 16-byte-per-lane copy kernel (the guide: 6.29 TB/s)
    assert 5000 < roof["measured_copy_GBps"] < 8000, roof["measured_copy_GBps"]
    assert out["legs"]["roofline"] == "done" and out["legs"]["cpu_baseline"].startswith("skipped")
    # configs[4]'s predictor at an interior rank's width on the library's own kernels, beside the PyTorch-ROCm route
    pred = out["predictor"]
    assert out["legs"]["predictor"] == "done" and pred["roofline"]["bound"] == "mfma", out["legs"]
    assert pred["ms_per_window"] < 1.5 and pred["speedup_vs_pytorch_rocm"] > 3, pred
    assert pred["max_difference_vs_pytorch_rocm_over_range"] < 1e-4, pred
    kernel_rate = 1028850 / (roof["us_per_step"] * 1e-6)
    assert out["value"] > kernel_rate / 1.5, (out["value"], kernel_rate)
    # the timed region is exactly the one call of --steps steps, and value / ms_per_step describe that call
    assert out["timed_calls"] == 1 and out["steps"] == 20
    assert abs(out["value"] - 1028850 * 1e3 / out["ms_per_step"]) < 1e-6 * out["value"]


def test_a_short_budget_takes_the_small_cpu_sample_and_says_so():
    """With little of the budget left the CPU baseline falls back from the 1M-tet mesh (25 s of assembly) to the 150k-tet
    sample and names the reason; the line still carries headline, roofline and parity, status 0."""
    out = _run("--gpus", "1", "--steps", "200", "--warmup", "20", "--budget-s", "75", "--full")
    assert out["legs"]["headline"] == "done" and out["legs"]["roofline"] == "done"
    base = out["cpu_baseline"]
    assert "fallback" in base and "n=10" in base["sample"] and base["value"] > 0
    assert out["parity"]["rel_l2"] < 1e-10 and "n=10" in out["parity"]["mesh"]
    assert out["leg_seconds"]["total"] < 75


def test_a_plain_run_times_exactly_its_steps_and_dumps_the_state(tmp_path):
    """Without --full the run is set-up, warm-up, ONE timed call of --steps steps and the line; --dump-outputs writes the
    state those steps computed (what get_state() hands a caller) as float64 .npy files."""
    out = _run("--gpus", "1", "--steps", "300", "--warmup", "30", "--dump-outputs", str(tmp_path / "dump"))
    assert out["legs"] == {"setup": "done", "headline": "done"}, out["legs"]
    assert out["steps"] == 300 and out["warmup"] == 30 and out["timed_calls"] == 1
    assert out["metric"] == "element_updates_per_s" and out["unit"] == "element-updates/s" and out["dtype"] == "f64"
    assert out["higher_is_better"] is True and out["ms_per_step"] > 0
    assert abs(out["value"] - 1028850 * 1e3 / out["ms_per_step"]) < 1e-6 * out["value"]
    for key in ("roofline", "per_gpu_of_8", "cache_exceeding", "unstructured", "predictor", "cpu_baseline", "parity"):
        assert key not in out, key
    files = sorted(os.listdir(tmp_path / "dump"))
    assert files == ["d0.npy", "dn.npy", "tn.npy"], files
    d0, dn, tn = (np.load(tmp_path / "dump" / f) for f in files)
    n_dof = 3 * 476 * 20 * 20  # the n = 19 beam: (25n + 1)(n + 1)^2 nodes
    assert d0.dtype == dn.dtype == tn.dtype == np.float64 and d0.shape == dn.shape == (n_dof, 1)
    assert np.isfinite(d0).all() and np.isfinite(dn).all() and np.abs(d0).max() > 0 and not np.array_equal(d0, dn)
    dt = float(out["config"]["workload"].rsplit("dt=", 1)[1])
    assert abs(float(tn) / dt - (30 + 8 + 300)) < 1e-3 * 338  # warm-up + the untimed call of 8 steps + the timed steps
