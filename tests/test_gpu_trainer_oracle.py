"""The trainer a user drives -- attach() -> AdapterDataParallel -> dp.step() / GraphedTrainStep -- against the fp64 oracle, three optimizer
steps per configuration (tests/trainer_oracle.py: the record, the comparison, the bounds; tests/test_trainer_oracle_host.py: the evidence
that the comparison can fail).  ``pytest -s`` prints the worst row of every check and the asserted preconditions."""
import pytest
import torch

from tests import trainer_oracle as T
from tests.trainer_oracle import Config, TrainerRun, failures

pytestmark = pytest.mark.gpu
K = 3


def _run(cfg, monkeypatch, tag, want=()):
    run = TrainerRun(cfg, monkeypatch)
    rows = run.run(K)
    print("\nTRAINER %s checks: %s" % (tag, T.summary([r for r in rows if not r.check.startswith("pre.")])))
    print("TRAINER %s preconditions: %s" % (tag, T.preconditions(rows)))
    have = {r.check for r in rows}
    base = {"y", "dx", "grad.kernel", "grad.hooked", "master", "state.work", "state.grad_left_zero", "state.t", "state.grad_none",
            "pre.term_over_base", "pre.base_over_term", "pre.no_cancel", "pre.m_over_g"}
    assert base | set(want) <= have, sorted((base | set(want)) - have)
    assert run.dp.optimizer.t == K
    bad = failures(rows)
    assert not bad, "%d rows past their bound:\n%s" % (len(bad), "\n".join(map(str, bad[:40])))
    return run, rows


def test_a_deferred_dA_two_micro_batches_clip_active(monkeypatch):
    run, _ = _run(Config(n_micro=2, defer_dA=True, max_grad_norm=T.CLIP_ACTIVE, clip_expect="active", weight_decay=0.01), monkeypatch, "a",
                  want=("clip.norm", "pre.clip_active", "state.shadow"))
    # 14 projections x 2 micro-batches x 3 steps left as problems of the per-layer batched dA_m launch; dB stays in the chain at rank pad 16
    assert run.batched == {"da": 14 * 2 * K, "db": 0}, run.batched


def test_b_no_deferral_one_micro_batch_clip_inactive_fused_forward(monkeypatch):
    run, _ = _run(Config(n_micro=1, defer_dA=False, max_grad_norm=T.CLIP_INACTIVE, clip_expect="inactive", n_kv_heads=4), monkeypatch, "b",
                  want=("clip.norm", "pre.clip_inactive", "state.shadow"))
    assert run.batched == {"da": 0, "db": 0}, run.batched


def test_c_rank_24_dropout_two_micro_batches(monkeypatch):
    run, _ = _run(Config(rank=24, n_micro=2, dropout=0.1), monkeypatch, "c", want=("state.shadow",))
    assert all(mb.spec.dropout_p == 0.1 and mb.spec.seed != 0 for c in run.rec.records for mb in c.members)


def test_d_rank_40_dB_travels_with_the_deferred_batch(monkeypatch):
    from moka_amd import _lib
    assert _lib.up_bwd_passes(40, _lib.MOKA_BF16) == 2 and _lib.rank_pad(40) == 64
    run, _ = _run(Config(rank=40), monkeypatch, "d", want=("state.shadow",))
    assert run.batched == {"da": 14 * K, "db": 14 * K}, run.batched


def test_e_vt_mirror_with_a_sample_without_image_tokens(monkeypatch):
    _run(Config(variant="vt"), monkeypatch, "e", want=("state.shadow", "grad.zero"))


def test_f_optimizer_in_backward_does_not_clip_and_says_so(monkeypatch):
    run, _ = _run(Config(opt_in_backward=True, n_buckets=2, max_grad_norm=1.0), monkeypatch, "f", want=("state.unclipped", "state.shadow"))
    assert run.dp.unclipped_steps == K


def test_g_without_persistent_shadows(monkeypatch):
    run, rows = _run(Config(persistent_shadows=False), monkeypatch, "g")
    assert not run.dp._shadowed and "state.shadow" not in {r.check for r in rows}


def test_h_fp32_storage(monkeypatch):
    _run(Config(dtype=torch.float32), monkeypatch, "h")


def test_i_checkpointed_layers_record_every_call_twice(monkeypatch):
    _run(Config(checkpoint=True), monkeypatch, "i", want=("ckpt.twice", "ckpt.x_equal", "state.shadow"))


@pytest.mark.parametrize("chains", [1, 2])
def test_jk_graphed_train_step(monkeypatch, chains):
    run, _ = _run(Config(graph_chains=chains), monkeypatch, "jk"[chains - 1], want=("state.shadow",))
    assert run.n_calls == 8 * chains                                   # 4 calls per layer (q+k+v, o, gate+up, down), 2 layers, per chain


def test_negative_control_shadows_that_are_not_refreshed_fail_the_second_steps_dx(monkeypatch):
    """The record and the comparison on the device have to be able to fail too: with refresh_shadows switched off behind attach() the
    kernels read BwT / AT of the initial weights -- step 1 computes what it should and leaves stale shadows, from step 2 on dx (through
    AT, and g through BwT) and the gradients that g feeds are wrong."""
    run = TrainerRun(Config(), monkeypatch)
    monkeypatch.setattr(run.dp, "refresh_shadows", lambda *a, **kw: None)
    rows = run.run(K)
    bad = failures(rows)
    print("\nTRAINER negative control: %s" % T.summary(bad))
    assert {r.check for r in failures(rows, step=1)} == {"state.shadow"}, failures(rows, step=1)[:8]
    assert failures(rows, "dx", step=2) and failures(rows, "grad.kernel", step=2) and failures(rows, "state.shadow", step=3)
    assert not failures(rows, "y") and not failures(rows, "master") and not failures(rows, "state.work"), "the forward and the optimizer read no shadow"
