"""The step bench.py times -- moka_amd.schedule.GraphedAdapterStep over bench.build_workload -- against the fp64 oracle
(tests/schedule_oracle.py): K real steps on tiny widths, every configuration that takes another path through the schedule's pre-built
argument lists, the tie to the real entry point, and negative controls (a kernel family left out must fail its check).

Bounds (all the project's own): y / dx relative Frobenius <= 1e-3 and <= 1 bf16 ulp per read-modify-write pass; every gradient view
<= 5e-5 (tests/test_gpu_parity.py); master <= 2e-6 against fp64 AdamW (tests/test_gpu_parallel.py); work, shadows, counters, the
gradient buffer left zero: exact.  Every test prints its report's worst row per check (pytest -s shows them).
"""
import importlib
import os
import subprocess
import sys

import pytest

from tests import schedule_oracle as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
bench = importlib.import_module("bench")


def _run(monkeypatch, widths, extra=(), K=3, skip=()):
    monkeypatch.setitem(bench.MODELS, "7b", H.WIDTHS[widths])
    run = H.ScheduleRun(list(H.BASE_ARGV) + list(extra), skip=skip)
    report = run.run(K)
    print("\n%s %s skip=%s: %d rows; %s" % (widths, " ".join(extra) or "defaults", ",".join(skip) or "-", len(report), H.summary(report)))
    return run, report


def _assert_clean(run, report, K=3):
    bad = H.failures(report)
    assert not bad, "%d failing rows, first: %s" % (len(bad), bad[:6])
    want = {"y.rel", "y.ulp", "dx.rel", "dx.ulp", "grad.dA", "grad.dB", "state.work"}
    if any(u.fused for u in run.plan.chains[0].units):
        want.add("state.shadow")
    assert want <= {r.check for r in report}
    assert {r.step for r in report} == set(range(1, K + 1))


def test_a_headline_schedule_uneven_chains(monkeypatch):
    """Defaults: avt, r 16, batch 3 as 2 + 1 sequences on two chains of one hub-shaped graph, dA_m per unit, fused forward, dropout 0.05,
    the AdamW slices inside the backward."""
    run, report = _run(monkeypatch, "mha")
    a = run.args
    assert (a.graph, a.chains, a.graph_topology, a.defer_da) == ("all", 2, "hub", "unit") and run.captured and run.sched.opt_in_bwd
    assert [c.B for c in run.plan.chains] == [2, 1] and all(u.fused for u in run.plan.chains[0].units)
    assert {"master", "state.t", "state.grad_left_zero", "epoch.distinct", "epoch.masks_differ", "pre.m_over_g", "pre.term_over_base"} <= {r.check for r in report}
    _assert_clean(run, report)


def test_capture_restores_the_flat_gradient(monkeypatch):
    """capture(restore_grad=True): the warm-up's dA_m / dB do not stay in the flat gradient -- a sentinel written in front of the capture
    comes back bit for bit -- so step 1's AdamW slices consume that step's gradient alone (grad.dA / grad.dB at step 1; with the
    warm-up's gradient left in they are 0.73 - 0.95 relative instead of <= 5e-5)."""
    import torch
    from moka_amd import schedule as SCH
    monkeypatch.setitem(bench.MODELS, "7b", H.WIDTHS["mha"])
    run = H.ScheduleRun(H.BASE_ARGV)
    assert run.captured and run.sched.opt_in_bwd and float(run.wl["gbuf"].abs().max()) == 0.0
    run.run(1)
    assert not H.failures(run.report, "grad") and not H.failures(run.report, "master"), H.failures(run.report)[:4]
    sentinel = torch.randn_like(run.wl["gbuf"])
    run.wl["gbuf"].copy_(sentinel)
    again = SCH.GraphedAdapterStep(run.wl, run.cfg, run.args.layers, optimizer=run.opt, world=1, comm=False, device=run.dev)
    assert again.capture(restore_grad=True) and torch.equal(run.wl["gbuf"], sentinel)
    run.wl["bucket"].zero_()


def test_b_layers_sharing_an_activation_set(monkeypatch):
    """Three layers over two activation sets: layers 0 and 2 add into the same y / dx (two passes per buffer of set 0)."""
    run, report = _run(monkeypatch, "mha", ["--layers", "3"])
    assert run.y_pass[(0, "q_proj")] == 2 and run.y_pass[(1, "q_proj")] == 1 and run.dx_pass[(0, "hid")] == 2
    _assert_clean(run, report)


def test_c_three_launch_unit_beside_fused_units(monkeypatch):
    """Grouped-query widths: q+k+v has unequal d_out, so the library advises the three-launch forward for it beside fused o / gate+up /
    down units; run_shadows skips the unit (its moka_cross_fwd writes its own shadows)."""
    run, report = _run(monkeypatch, "gqa")
    fused = {"+".join(m.name for m in u.members): u.fused for u in run.plan.chains[0].units}
    assert fused["q_proj+k_proj+v_proj"] is False and fused["o_proj"] and fused["gate_proj+up_proj"] and fused["down_proj"]
    _assert_clean(run, report)


def test_d_one_chain_batched_da_per_layer(monkeypatch):
    """--chains 1: chain topology, a layer's dA_m as one moka_down_bwd_da_batch launch (make_layer_batches), bucket_opt slices on the side stream."""
    run, report = _run(monkeypatch, "mha", ["--chains", "1"])
    assert (run.args.graph_topology, run.args.defer_da) == ("chain", "layer") and run.captured
    _assert_clean(run, report)


def test_e_rank_64_split_db(monkeypatch):
    """Rank 64: no fused forward, dB a pass of its own off the chain (moka_up_bwd_db_batch)."""
    run, report = _run(monkeypatch, "mha", ["--rank", "64", "--batch", "2", "--chains", "1"])
    assert run.args.split_db and not any(u.fused for u in run.plan.chains[0].units)
    _assert_clean(run, report)


def test_f_visual_text_variant(monkeypatch):
    """--variant vt: two modalities, s_in / s_out in swapped roles, w = 0.05."""
    run, report = _run(monkeypatch, "mha", ["--variant", "vt"])
    assert run.plan.M == 2 and run.plan.s_in == 1.0
    _assert_clean(run, report)


@pytest.mark.parametrize("extra", [("--graph", "off"), ("--graph", "bwd", "--buckets", "2"), ("--no-optimizer",), ("--dropout", "0"), ("--defer-da", "bucket")],
                         ids=lambda e: " ".join(e))
def test_g_other_paths(monkeypatch, extra):
    """Live launches; per-bucket graphs with the optimizer behind them; the gradient read directly; no masks; held layers."""
    run, report = _run(monkeypatch, "mha", extra)
    if extra[:2] == ("--graph", "off"):
        assert not run.captured
    else:
        assert run.captured
    if extra == ("--no-optimizer",):
        assert run.opt is None and "master" not in {r.check for r in report}
    if extra == ("--dropout", "0"):
        assert run.wl["seed_epoch"] is None
    _assert_clean(run, report)


def test_h_the_harness_builds_the_step_bench_times(tmp_path):
    """Real 7B widths: bench.py --dump-outputs as a subprocess against the same arguments through the harness in-process (no scaling, a
    plain capture(), nothing put back behind it): y / dx bit-identical, the gradient to the spread of its atomics -- the harness's copy
    of main's resolution builds the step bench.py times.  The in-process run also passes the oracle checks, of which only the gradient
    and state rows carry weight here: the buffers are unscaled, so the adapter term is below one bf16 ulp of the N(0, 1) base and the
    y / dx rows cannot see it (no y / dx coverage at 7B widths is claimed; configurations a-g carry that)."""
    import numpy as np
    argv = ["--gpus", "1", "--layers", "2", "--batch", "2", "--seq", "256", "--distinct", "2", "--no-optimizer", "--warmup", "1", "--steps", "2"]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv, "--dump-outputs", str(tmp_path / "a")],
                         capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-3000:]
    run = H.ScheduleRun(argv, bench_exact=True)
    report = run.run(3)                                                          # warm-up 1 + 2 timed steps
    print("\n7b widths: %d rows; %s" % (len(report), H.summary(report)))
    bench.dump_outputs(bench.step_outputs(run.wl, False), str(tmp_path / "b"))
    a = {f: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    b = {f: np.load(tmp_path / "b" / f) for f in sorted(os.listdir(tmp_path / "b"))}
    assert set(a) == set(b) and "grad.npy" in a and sum(f.startswith("y.") for f in a) == 28 and sum(f.startswith("dx.") for f in a) == 16
    for f in a:
        if f != "grad.npy":
            assert np.array_equal(a[f], b[f]), f
    assert float(np.abs(a["grad.npy"] - b["grad.npy"]).max()) <= 2e-5 * float(np.abs(a["grad.npy"]).max())     # fp32 atomics in a different order
    _assert_clean(run, report)


# what the report must flag when a kernel family is left out of the schedule (ScheduleConfig.skip: results wrong by construction)
MUST_FIRE = {"down_fwd": "y", "up_fwd": "y", "up_bwd": "dx", "cross_bwd": "dx", "dx": "dx", "dA": "grad.dA", "shadows": "state.shadow", "optimizer": "master"}


def test_negative_controls_cover_every_family():
    from moka_amd.schedule import FAMILIES
    assert set(MUST_FIRE) == set(FAMILIES) - {"none"}


@pytest.mark.parametrize("family", sorted(MUST_FIRE))
def test_i_a_skipped_family_fails_its_check(monkeypatch, family):
    """Configuration a, two steps, one family's launches left out (as bench.py --ablate does): a harness that passes it is broken."""
    run, report = _run(monkeypatch, "mha", K=2, skip=(family,))
    fired = H.failures(report, MUST_FIRE[family], step=2 if family == "shadows" else None)
    assert fired, (family, MUST_FIRE[family], sorted({r.check for r in H.failures(report)}))
