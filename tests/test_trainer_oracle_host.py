"""The comparison half of tests/trainer_oracle.py has to be able to fail (no GPU): a correct step emulated on the CPU gives no failing row,
every seeded fault gives failing rows of the check that names it and of no unrelated check.  Also: the restated HF no-decay rule against
transformers, the restated layout against a CPU attach(), and the scales / clip thresholds the GPU tests run with, from the fp64 model."""
import math

import pytest
import torch

from tests import trainer_oracle as T
from tests.trainer_oracle import FAULTS, StepCfg, ToyTrainer, failures

ACTIVE = StepCfg(lr=1e-2, weight_decay=0.01, max_grad_norm=1.0, clip_expect="active")
INACTIVE = StepCfg(lr=1e-2, weight_decay=0.01, max_grad_norm=1000.0, clip_expect="inactive")
NO_CLIP = StepCfg(lr=1e-2, weight_decay=0.01)


@pytest.mark.parametrize("cfg", [ACTIVE, INACTIVE, NO_CLIP, ACTIVE._replace(world=2), NO_CLIP._replace(world=2)],
                         ids=["clip_active", "clip_inactive", "no_clip", "world2_clip", "world2"])
def test_a_correct_step_gives_no_failing_row(cfg):
    rows = ToyTrainer(cfg).run(3)
    print(T.summary(rows))
    assert not failures(rows), failures(rows)
    have = {r.check for r in rows}
    assert {"y", "dx", "grad.kernel", "grad.hooked", "pad", "master", "state.work", "state.shadow", "state.grad_left_zero", "state.t",
            "pre.term_over_base", "pre.base_over_term", "pre.no_cancel", "pre.m_over_g"} <= have
    if cfg.max_grad_norm is not None:
        assert {"clip.norm", "pre.clip_" + cfg.clip_expect} <= have


# fault -> (configuration, checks that must fail, further checks that may, parameters the failing gradient / master rows are confined to)
SEEDED = {
    "micro_batch_missing": (ACTIVE, {"grad.kernel", "grad.hooked"}, {"clip.norm"}, None),
    "sum_not_mean": (NO_CLIP._replace(world=2), {"grad.kernel", "grad.hooked"}, set(), None),
    "clip_from_sum_norm": (ACTIVE._replace(world=2), {"grad.kernel", "grad.hooked"}, set(), None),
    "clip_not_clamped": (INACTIVE, {"grad.kernel", "grad.hooked"}, set(), None),
    "clip_kernel_fed_only": (ACTIVE, {"grad.hooked"}, {"pre.m_over_g"}, None),     # (the unclipped first moments are 100 x the clipped gradient)
    "decay_on_norm": (NO_CLIP, {"master"}, set(), {"norm.weight"}),
    "decay_ignores_padding": (NO_CLIP, {"master"}, set(), None),
    "dA1_in_dA2": (NO_CLIP, {"grad.kernel"}, set(), {"p0.lora_A1.weight", "p0.lora_A2.weight"}),
    "stale_AT": (NO_CLIP, {"state.shadow", "dx"}, set(), None),
    "work_truncated": (NO_CLIP, {"state.work"}, set(), None),
    "bias_correction_lags": (NO_CLIP, {"master"}, set(), None),
}


def test_every_fault_of_the_list_is_seeded():
    assert set(SEEDED) == set(FAULTS)


@pytest.mark.parametrize("fault", FAULTS)
def test_a_seeded_fault_fails_the_check_that_names_it_and_no_unrelated_one(fault):
    cfg, must, may, where = SEEDED[fault]
    rows = ToyTrainer(cfg, fault=fault).run(3)
    bad = failures(rows)
    got = {r.check for r in bad}
    assert must <= got <= must | may, (fault, sorted(got), bad[:6])
    assert not any(r.check.startswith("pre.") and r.check != "pre.m_over_g" for r in bad), "the other preconditions come from the oracle alone"
    if where is not None:
        assert {r.where for r in bad} == where, (fault, sorted({r.where for r in bad}))
    if fault == "stale_AT":
        assert not failures(rows, "dx", step=1) and failures(rows, "dx", step=2), "a stale AT shows in the SECOND step's dx"
    if fault == "bias_correction_lags":
        assert not failures(rows, step=1) and len(failures(rows, "master", step=2)) == len(ToyTrainer(cfg).views)
    if fault == "decay_ignores_padding":
        # the ranges move by the padding in front of them: the bias (no decay) and the norm weight are cut through
        assert {"proj.bias", "norm.weight"} & {r.where for r in bad}


def test_a_wrong_coefficient_is_a_uniform_ratio():
    """clip_from_sum_norm at world 2 halves every gradient: every grad row is off by the same 0.5."""
    rows = ToyTrainer(ACTIVE._replace(world=2), fault="clip_from_sum_norm").run(1)
    vals = [r.value for r in rows if r.check in ("grad.kernel", "grad.hooked")]
    assert vals and all(abs(v - 0.5) < 1e-3 for v in vals), vals


# ---------------------------------------------------------------------------------------------------------------------------------------
# the restatements against what they restate
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,dtype", [("avt", torch.bfloat16), ("vt", torch.bfloat16), ("avt", torch.float32)])
def test_layout_restatement_equals_a_cpu_attach(variant, dtype):
    from moka_amd.parallel import attach
    m = T.TrainerLM("cpu", dtype, variant)
    views = T.expected_layout(m)
    nd = T.hf_no_decay(m)
    dp = attach(m, n_buckets=2, optimizer=False)
    try:
        assert [(v.name, v.offset, v.size) for v in views] == list(zip(dp.names, dp.offsets, dp.sizes))
        assert {v.name for v in views if v.kernel} == set(dp.kernel_fed) and {v.name for v in views if not v.kernel} == set(dp.hooked)
        assert dp.bucket.flat.numel() == views[-1].padded_end
        # the hooked no-decay parameters sit between a decaying one and the adapters: a no-decay range in the middle of the buffer
        flags = [v.decay for v in views]
        first = flags.index(False)
        assert first > 0 and not all(flags[first:]) and any(flags[first:])
        assert {v.name for v in views if not v.decay} == {"vl_projector.bias", "model.layers.1.input_layernorm.weight",
                                                           "model.layers.1.post_attention_layernorm.weight"} == nd & {v.name for v in views}
    finally:
        dp.detach()


def test_no_decay_restatement_equals_transformers():
    transformers = pytest.importorskip("transformers")
    m = T.TrainerLM("cpu", torch.bfloat16, "avt")
    for p in m.parameters():
        p.requires_grad = True                    # (the rule is about module types and names, not about what is trainable)
    tr = transformers.Trainer.__new__(transformers.Trainer)
    decay = set(transformers.Trainer.get_decay_parameter_names(tr, m))
    names = {n for n, _ in m.named_parameters()}
    assert names - decay == T.hf_no_decay(m)


# ---------------------------------------------------------------------------------------------------------------------------------------
# scales and clip thresholds, from the fp64 model alone
# ---------------------------------------------------------------------------------------------------------------------------------------
REFERENCE_CONFIGS = [("avt", 8, 2), ("avt", 24, 2), ("avt", 40, 2), ("vt", 8, 2), ("avt", 8, 4)]


@pytest.mark.parametrize("variant,rank,kv", REFERENCE_CONFIGS)
def test_scales_and_clip_thresholds_hold_in_the_fp64_model(variant, rank, kv):
    m = T.TrainerLM("cpu", torch.float32, variant, rank, n_kv_heads=kv)
    norms = []
    for k, i in ((1, 0), (1, 1), (3, 0)):
        batch = T.make_batch(10 * k + i, {1: 2, 3: 3}[k] + i, no_image_sample=1 if variant == "vt" else None, dtype=torch.float32)
        ratios = []
        loss, params = T.reference_loss(m, batch, ratios)
        assert len(ratios) == 14
        print(variant, rank, "term / base %.3f .. %.3f" % (min(ratios), max(ratios)))
        assert 0.5 <= min(ratios) and max(ratios) <= 2.0, ratios
        names = [n for n in params]
        grads = torch.autograd.grad(loss, [params[n] for n in names], allow_unused=True)
        norms.append(math.sqrt(sum(float(g.pow(2).sum()) for g in grads if g is not None)))
    print(variant, rank, "gradient norm", norms)
    # clip active: coefficient < 0.7 also for the mean of two micro-batches that do not cancel (norm >= half of one); inactive: norm < half
    assert T.CLIP_ACTIVE / (0.5 * min(norms)) < 0.7 and max(norms) < 0.5 * T.CLIP_INACTIVE
