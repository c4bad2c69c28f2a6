"""The schedules bench.py captures (part-batch chains on forked streams, deferred dA_m on the hub, per-bucket graphs) compute what
the same launches compute live on one stream: `bench.py --verify-graph` (graph replay vs live, from the same activation state).
Correctness of that step against the fp64 oracle: tests/test_gpu_schedule_oracle.py."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _bench(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--layers", "5", "--seq", "512", "--steps", "2", "--warmup", "1",
                          "--full", "--no-cpu-baseline", "--no-traffic", "--no-optimizer", "--verify-graph", *extra],
                         capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.parametrize("extra", [
    (),                                                   # the default: 2 chains, hub-shaped one-graph step, dA_m one launch per layer
    ("--defer-da", "side"),
    ("--defer-da", "layer"),
    ("--defer-da", "bucket"),
    ("--defer-da", "off"),
    ("--chains", "4"),
    ("--chains", "1"),                                    # round 4's shape with the chain-first capture order
    ("--chains", "1", "--graph-topology", "hub"),
    ("--graph", "bwd"),                                   # what N > 1 replays: forward graph + one graph per gradient bucket, 2 chains
    ("--graph", "bwd", "--chains", "1"),
    ("--rank", "64", "--batch", "2", "--chains", "2"),    # dB off the chain too (a pass of its own at this rank)
    ("--variant", "vt"),
], ids=lambda e: " ".join(e) or "default")
def test_captured_schedule_equals_live_launches(extra):
    out = _bench(*extra)
    chk = out["graph_check"]
    assert chk is not None and chk["tensors_compared"] > 0
    assert chk["activations_bit_identical"], (extra, chk)
    assert chk["grad_nonzero_frac"] > 0.9 and chk["grad_max_abs"] > 0
    assert chk["grad_max_abs_diff_over_max"] <= 2e-5, (extra, chk)        # fp32 atomics in a different order
    if "--chains" not in extra and "--rank" not in extra:
        assert out["chains"] == 2


def test_default_line_says_how_it_ran():
    out = _bench()
    assert out["graph"] == "all" and out["graph_topology"] == "hub" and out["chains"] == 2 and out["defer_dA"] in ("layer", "side", "unit")
    assert "attach" in out["schedule"] and "--e2e" in out["schedule"]      # whose schedule the headline is (and which flag measures the autograd path)


def test_capture_failure_falls_back_to_live_launches_of_every_chain():
    """hipGraph capture is an optimisation: when it fails the step is launched live -- with two chains, both part-batches back to back on the
    one stream (it used to run only the first chain's launches; then it exited).  MOKA_BENCH_FAIL_CAPTURE=1 is the test hook."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    outs = {}
    for name, extra_env, extra in (("graph", {}, ()), ("fallback", {"MOKA_BENCH_FAIL_CAPTURE": "1"}, ()), ("off", {}, ("--graph", "off", "--chains", "2"))):
        res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--layers", "4", "--seq", "512", "--steps", "3", "--warmup", "1",
                              "--full", "--no-cpu-baseline", "--no-traffic", *extra], capture_output=True, text=True, timeout=900, env={**env, **extra_env}, cwd=ROOT)
        assert res.returncode == 0, res.stderr[-3000:]
        lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        outs[name] = json.loads(lines[0])
        if name == "fallback":
            assert "launching live" in res.stderr and "2 chains back to back" in res.stderr
    assert outs["graph"]["chains"] == outs["fallback"]["chains"] == outs["off"]["chains"] == 2
    # the same launches, the same bytes: the per-pass entry-point table (taken from live passes in every mode) covers both chains
    for k in ("moka_up_fwd", "moka_down_bwd"):
        a, b = outs["graph"]["entry_point_ms_per_pass"][k], outs["fallback"]["entry_point_ms_per_pass"][k]
        assert a > 0 and b > 0 and 0.5 < a / b < 2.0
    assert outs["fallback"]["value"] > 0 and outs["off"]["value"] > 0 and outs["graph"]["value"] >= 0.8 * outs["fallback"]["value"]


@pytest.mark.parametrize("extra", [(), ("--chains", "1"), ("--defer-da", "layer")], ids=lambda e: " ".join(e) or "default")
def test_default_schedule_with_optimizer_equals_live_steps(extra):
    """the headline schedule WITH its optimizer -- two chains sharing gradient accumulators, AdamW slices and weight-shadow
    rewrites on the hub behind per-branch events -- was never compared against live launches.  `bench.py --verify-graph` (without
    --no-optimizer): 3 steps as the captured graph and 3 steps live from identical master / moments / activations."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--layers", "5", "--seq", "512", "--steps", "2", "--warmup", "1",
                          "--full", "--no-cpu-baseline", "--no-traffic", "--verify-graph", *extra], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-3000:]
    out = json.loads([l for l in res.stdout.splitlines() if l.startswith("{")][0])
    chk = out["graph_check"]
    assert chk["steps"] == 3 and chk["grad_left_zero"], chk
    assert chk["master_rel_diff"] <= 1e-5, chk                     # (fp32 atomics in a different order: last bits of the gradients)
    assert chk["work_max_abs_diff"] <= 1e-3 and chk["shadow_max_abs_diff"] <= 1e-3, chk       # bf16 copies: an ulp where the master's last bits differ
    assert chk["activations_max_rel_diff"] <= 1e-3, chk


def _plain(dump, *extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", "--layers", "2", "--seq", "512",
                          "--dump-outputs", str(dump), *extra], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    return json.loads(lines[0])


def _load(d):
    import numpy as np
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    """A plain run times exactly --steps steps and measures nothing else (no roofline passes, no CPU baseline: --full); --dump-outputs writes
    what the last timed step left for its caller, float32, at most 64 MB; the same arguments give the same inputs, so without the optimizer
    (the weights then stay as built) two runs compute the same y / dx and, up to the order of fp32 atomics, the same gradient."""
    import numpy as np
    out = _plain(tmp_path / "a")
    assert out["steps"] == 3 and out["warmup"] == 2 and out["full"] is False
    assert out["unit"] == "tokens/s" and out["higher_is_better"] is True and out["dtype"] == "bf16" and out["metric"].startswith("tokens/sec/GPU")
    assert out["ms_per_step"] > 0 and abs(out["value"] - 4 * 512 * 1e3 / out["ms_per_step"]) <= 1e-2 * out["value"]
    for k in ("roofline", "kernels", "entry_point_ms_per_pass", "cpu_baseline", "graph_replay_host_ms", "ablation"):
        assert k not in out, k
    d = _load(tmp_path / "a")
    assert {"y.chain0.set0.q_proj", "y.chain1.set1.down_proj", "dx.chain0.set0.hid", "dx.chain1.set1.act", "params"} <= set(d)
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in d.values())
    assert sum(os.path.getsize(os.path.join(tmp_path / "a", f)) for f in os.listdir(tmp_path / "a")) <= 64 * 10 ** 6
    runs = []
    for name in ("b", "c"):
        _plain(tmp_path / name, "--no-optimizer")
        runs.append(_load(tmp_path / name))
    b, c = runs
    assert set(b) == set(c) and "grad" in b and "params" not in b
    for k in b:
        rel = float(np.linalg.norm(b[k].astype(np.float64) - c[k]) / max(np.linalg.norm(b[k].astype(np.float64)), 1e-30))
        assert rel <= (1e-5 if k == "grad" else 1e-6), (k, rel)
    assert float(np.abs(b["grad"]).max()) > 0
