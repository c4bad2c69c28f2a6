"""The pure parts of tests/schedule_oracle.py (no GPU): the fp64 AdamW reference, the gradient recovered from two consecutive fp32 first
moments, the counter of read-modify-write passes per buffer, and the report machinery the GPU tests assert on.  The last test
(the harness's copy of bench.main's `auto` resolution) asks the built library for moka_up_bwd_passes, like tests/test_capi_symbols.py:
it needs build(), not a GPU.

Bounds of this file that are not quoted from another test, and where they come from: 1e-13 for two fp64 evaluations of one formula
(number format: a few hundred ulps of 2^-53); 2e-6 for the recovered gradient (the issue's figure); 2 % on the norm ratio of the
synthetic first moment and > 0.4 for the wrong-scale control are checks of the test's own construction, not of code under test."""
import pytest
import torch

from tests import schedule_oracle as H


@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_fp64_adamw_reference_is_the_torch_formula(wd):
    """Five steps on fp64 CPU tensors against torch.optim.AdamW: the two evaluate the same formula in fp64 in a different operation order,
    so they agree to fp64 rounding (1e-13 relative: some hundred ulps of 2^-53 for five steps of a dozen operations each)."""
    g = torch.Generator().manual_seed(3)
    p0 = torch.randn(4099, generator=g, dtype=torch.float64) * 0.02
    ref_p = torch.nn.Parameter(p0.clone())
    ref = torch.optim.AdamW([ref_p], lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    for t in range(1, 6):
        grad = torch.randn(4099, generator=g, dtype=torch.float64) * (0.1 * t)
        ref_p.grad = grad.clone()
        ref.step()
        p, m, v = H.adamw_fp64(p, m, v, grad, t, 1e-4, (0.9, 0.999), 1e-8, wd)
        assert H.rel(p, ref_p.data) <= 1e-13, (t, H.rel(p, ref_p.data))
    st = ref.state[ref_p]
    assert H.rel(m, st["exp_avg"]) <= 1e-13 and H.rel(v, st["exp_avg_sq"]) <= 1e-13
    assert float((p - p0).abs().max()) > 1e-5                    # (the five steps moved the parameters)


@pytest.mark.parametrize("ratio", [0.0, 0.5, 2.0])
def test_gradient_recovered_from_two_first_moments(ratio):
    """m_k = fma(beta1, m_{k-1}, (1 - beta1) * scale * g) in fp32, as moka_adamw_kernel evaluates it: the gradient recovered in fp64 from
    m_{k-1} and m_k is within 2e-6 (relative Frobenius) of g for |m_{k-1}| / |g| up to 2 -- the precondition the harness asserts."""
    gen = torch.Generator().manual_seed(11)
    n = 1 << 16
    g = (torch.randn(n, generator=gen) * 3e-3).float()
    m_old = (torch.randn(n, generator=gen).float() * (ratio * g.norm() / (n ** 0.5))).float()
    if ratio:
        assert abs(m_old.norm().item() / g.norm().item() - ratio) < 0.02 * ratio
    b1, omb1 = H.f32_beta(0.9)
    scale = 0.5
    gs = (g.double() * scale).float()                                            # g *= grad_scale
    t = (omb1 * gs.double()).float()                                             # (1.f - beta1) * g
    m_new = (b1 * m_old.double() + t.double()).float()                           # fmaf: one rounding
    rec = H.recover_grad(m_new, m_old, 0.9, scale)
    assert H.rel(rec, g) <= 2e-6, H.rel(rec, g)
    assert H.rel(H.recover_grad(m_new, m_old, 0.9, 1.0), g) > 0.4                # (the scale matters)


def test_pass_counter_groups_no_group_and_shared_sets():
    U = H.UnitDesc
    layer = lambda s: [U(s, "hid", ("q_proj", "k_proj", "v_proj")), U(s, "attn", ("o_proj",)), U(s, "hid2", ("gate_proj", "up_proj")),   # noqa: E731
                       U(s, "act", ("down_proj",))]
    # two layers, two sets, grouped: every buffer one pass (a group is ONE pass over its shared dx)
    y, dx = H.count_passes(layer(0) + layer(1))
    assert set(y.values()) == {1} and set(dx.values()) == {1} and len(y) == 14 and len(dx) == 8
    # --no-group: q / k / v are units of their own -> three passes over dx of hid, two over dx of hid2; y still one each
    single = [U(0, "hid", ("q_proj",)), U(0, "hid", ("k_proj",)), U(0, "hid", ("v_proj",)), U(0, "attn", ("o_proj",)),
              U(0, "hid2", ("gate_proj",)), U(0, "hid2", ("up_proj",)), U(0, "act", ("down_proj",))]
    y, dx = H.count_passes(single)
    assert dx == {(0, "hid"): 3, (0, "attn"): 1, (0, "hid2"): 2, (0, "act"): 1} and set(y.values()) == {1}
    # three layers over two sets: layers 0 and 2 share set 0 -> two passes over each of its buffers
    y, dx = H.count_passes(layer(0) + layer(1) + layer(0))
    assert y[(0, "q_proj")] == 2 and y[(1, "q_proj")] == 1 and dx[(0, "hid")] == 2 and dx[(1, "act")] == 1
    y, dx = H.count_passes(single + layer(1) + single)
    assert dx[(0, "hid")] == 6 and dx[(1, "hid")] == 1 and y[(0, "k_proj")] == 2


def test_report_flags_a_planted_discrepancy():
    R = [H.Row(1, "y.rel", "y.chain0.set0.q_proj", 3e-4, 1e-3), H.Row(1, "y.ulp", "y.chain0.set0.q_proj", 1.0, 1.0 + 1e-6),
         H.Row(2, "grad.dA", "L0.q_proj.dA1", 1e-6, 5e-5), H.Row(2, "state.shadow", "L1.o_proj", 0.0, 0.0)]
    assert not H.failures(R)
    R.append(H.Row(2, "state.shadow", "L0.o_proj", 17.0, 0.0))                 # a stale shadow
    R.append(H.Row(2, "grad.dA", "L0.k_proj.dA0", float("nan"), 5e-5))         # a NaN never passes
    R.append(H.Row(1, "y.ulp", "y.chain1.set0.v_proj", 2.0, 1.0 + 1e-6))
    assert [r.where for r in H.failures(R)] == ["L0.o_proj", "L0.k_proj.dA0", "y.chain1.set0.v_proj"]
    assert [r.where for r in H.failures(R, "y")] == ["y.chain1.set0.v_proj"] and not H.failures(R, "dx") and not H.failures(R, "grad.dB")
    assert len(H.failures(R, "state.shadow", step=2)) == 1 and not H.failures(R, "state.shadow", step=1)
    w = H.worst(R)
    assert w["state.shadow"].where == "L0.o_proj" and w["grad.dA"].where == "L0.k_proj.dA0" and w["y.rel"].value == 3e-4
    assert "state.shadow 17 / 0" in H.summary(R)


def test_resolution_of_the_auto_fields_for_the_default_configuration(monkeypatch):
    """The harness's copy of bench.main's resolution on the tiny widths: the headline shape (two chains, one hub-shaped graph, dA_m per unit)."""
    import importlib
    bench = importlib.import_module("bench")
    monkeypatch.setitem(bench.MODELS, "7b", H.WIDTHS["mha"])
    a = H.resolve_args(H.BASE_ARGV)
    assert (a.graph, a.chains, a.graph_topology, a.defer_da, a.hub, a.chain_priority, a.split_db) == ("all", 2, "hub", "unit", True, "high", False)
    a = H.resolve_args(H.BASE_ARGV + ["--chains", "1"])
    assert (a.graph_topology, a.defer_da, a.hub) == ("chain", "layer", False)
    a = H.resolve_args(H.BASE_ARGV + ["--rank", "64", "--batch", "2", "--chains", "1"])
    assert a.split_db is True and a.chain_priority == "normal"
    a = H.resolve_args(H.BASE_ARGV + ["--graph", "off"])
    assert (a.chains, a.defer_da, a.hub) == (1, "layer", False)
