"""CPU: the regime generator of tests/interaction_regimes.py delivers what it claims, the float32 emulation of the kernels' blocking
passes every regime with at least 4x margin, and every mutant of the emulation is rejected by the same checks by more than 10x.
This is the evidence that tests/test_gpu_interaction_regimes.py fails when a kernel is subtly wrong."""
import math

import pytest
import torch

from tests import interaction_regimes as IR

REGS = IR.regimes()
_DATA = {}


def _data(reg):
    if reg.id not in _DATA:
        _DATA[reg.id] = IR.make(reg)
    return _DATA[reg.id]


def _slot_live(d, b):
    return d.ort.kvalid[b] & (d.ort.tok_mod[b, d.ort.kpos[b]] >= 0)


def test_the_regimes_cover_the_issue_matrix():
    lks, rs, ws, kss, Ls = set(), set(), set(), set(), set()
    overlap_rp = set()
    for reg in REGS:
        d = _data(reg)
        assert reg.S % 16 and reg.S % 128, f"{reg.id}: S = {reg.S} is a multiple of 16"
        rs.add(reg.r)
        ws.add(reg.w)
        kss.add(reg.ks)
        for b in range(d.B):
            Lk = int(d.rt.klen[b])
            lks.add(Lk)
            Ls.add(round(reg.samples[b].L))
            rows = torch.arange(b * d.S, (b + 1) * d.S)
            if Lk > 64 and bool((d.is_query[rows] & d.is_key[rows]).any()):
                overlap_rp.add(d.RP)
    assert {1, 15, 16, 17, 33, 49, 63, 64, 65, 127, 128, 129, 200, 600} <= lks
    assert 0 in lks                                                        # samples without keys
    assert {4, 12, 16, 20, 32, 48, 64} <= rs and {0.05, 1.0, -1.0, 4.0} <= ws and {1, 3, 7} <= kss
    assert {0, 3, 30, 120, 600} <= Ls
    assert overlap_rp == {16, 32, 64}                                      # query rows that are key rows, Lk > 64, every rank pad
    assert any(abs(reg.inv_sqrt_dk - 1 / math.sqrt(reg.r)) > 1e-3 for reg in REGS)
    assert max(len(reg.samples) for reg in REGS) == 8
    # 128-token blocks of the fused kernel that span more than one sample
    assert any(len(reg.samples) * reg.S > 128 and 128 % reg.S and reg.S < 128 for reg in REGS)
    # a sample without query rows that has keys (AVT) and one with queries but no keys (VT)
    assert any(int(_data(reg).rt.klen[b]) > 0 and not bool(_data(reg).ort.is_query[b].any()) for reg in REGS for b in range(len(reg.samples)))


@pytest.mark.parametrize("reg", REGS, ids=[r.id for r in REGS])
def test_the_generator_delivers_what_it_claims(reg):
    d = _data(reg)
    # inputs: exact slices, NaN rows of no modality, zero pad columns
    assert torch.isnan(d.part[:, ~d.has_mod]).all() and torch.isnan(d.g_part[:, ~d.has_mod]).all()
    assert torch.equal(d.part[:, d.has_mod].sum(0), d.h[d.has_mod]) and torch.equal(d.part[:, d.has_mod].flip(0).sum(0), d.h[d.has_mod])
    assert torch.equal(d.g_part[:, d.has_mod].sum(0), d.g[d.has_mod])
    if d.RP > d.r:
        assert float(d.part[:, d.has_mod, d.r:].abs().max()) == 0.0
    for b, smp in enumerate(reg.samples):
        lg = d.logits[b]
        Lk = int(d.rt.klen[b])
        if lg is None:
            continue
        live = _slot_live(d, b)
        if smp.mode == "zeroq":
            assert float(lg.abs().max()) == 0.0
            continue
        assert abs(d.L[b] - smp.L) <= 0.05 * smp.L + 1e-9, (b, d.L[b], smp.L)
        qrows = torch.where(d.ort.is_query[b])[0]
        am = lg.argmax(1)[~d.is_key[b * d.S + qrows]]        # (a query row that is a key row carries the key pattern)
        if smp.mode in ("first", "last", "at"):
            j = {"first": 0, "last": Lk - 1, "at": smp.at}[smp.mode]
            assert bool((am == j).all()), (b, smp.mode, am.unique())
            if smp.mode == "last" and Lk % 64 == 1:
                assert j == Lk - 1 and j % 64 == 0                                  # the lone key of the last chunk
        if smp.mode == "rise":
            assert bool((am == Lk - 1).all())
            row = lg[int(torch.where(~d.is_key[b * d.S + qrows])[0][0])]
            tiles = [float(row[j0:j0 + 16].max()) for j0 in range(0, Lk, 16)]
            assert all(y > x for x, y in zip(tiles, tiles[1:]))                    # the running max rises in every later tile / chunk
        if smp.mode == "equal":
            assert float((lg - lg[:, :1]).abs().max()) <= 1e-9 * max(1.0, d.L[b])  # uniform P
        if smp.mode == "neg":
            assert float(lg[:, live].max()) <= -40.0
            P = torch.softmax(lg, -1)
            assert float(P[:, ~live].sum(1).min()) > 0.99                           # the zero key rows hold > 99 % of the mass
        if smp.mode == "allneg":
            assert bool(live.all()) and float(lg.max()) <= -0.7 * smp.L


def test_waves_without_keys_occur_at_peaked_logits():
    short, tail = False, False
    for reg in REGS:
        d = _data(reg)
        for b in range(d.B):
            Lk = int(d.rt.klen[b])
            if d.logits[b] is None or d.L[b] < 100:
                continue
            short |= 0 < Lk <= 48
            tail |= Lk > 64 and 1 <= Lk % 64 <= 48
    assert short and tail


@pytest.mark.parametrize("reg", REGS, ids=[r.id for r in REGS])
def test_the_fp32_emulation_passes_with_margin(reg):
    d = _data(reg)
    hp = IR.emulate_forward(d)
    dh = IR.emulate_backward(d)
    IR.check_forward_exact(d, hp)
    IR.check_backward_exact(d, dh)
    fe, be = IR.forward_errors(d, hp), IR.backward_errors(d, dh)
    assert fe and be
    assert IR.worst(fe) <= 0.25, IR.fmt(fe)
    assert IR.worst(be) <= 0.25, IR.fmt(be)


@pytest.mark.parametrize("mut", IR.MUTANTS)
def test_every_mutant_is_rejected(mut):
    worst = 0.0
    for reg in REGS:
        d = _data(reg)
        worst = max(worst, IR.worst(IR.forward_errors(d, IR.emulate_forward(d, mut=(mut,)))),
                    IR.worst(IR.backward_errors(d, IR.emulate_backward(d, mut=(mut,)))))
    assert worst >= 10.0, f"{mut}: worst err / bound = {worst:.3g}"


def test_the_oracle_interaction_matches_autograd():
    """interaction_backward of oracle/moka_oracle.py against autograd of interaction_forward, on an overlap regime."""
    from oracle import moka_oracle as O
    d = _data(next(r for r in REGS if r.id == "vt_r8_overlap"))
    h = d.h[:, :d.r].double().reshape(d.B, d.S, d.r).clone().requires_grad_(True)
    ia = O.interaction_forward(h, d.ort, d.reg.w, d.reg.inv_sqrt_dk)
    g = d.g[:, :d.r].double().reshape(d.B, d.S, d.r)
    (ia.hp * g).sum().backward()
    dh, dq, dk = O.interaction_backward(g, O.interaction_forward(h.detach(), d.ort, d.reg.w, d.reg.inv_sqrt_dk))
    assert torch.allclose(dh, h.grad, rtol=1e-10, atol=1e-10)
    assert torch.equal(dh, g + dq + dk)
    both = (d.is_query & d.is_key).reshape(d.B, d.S)
    assert both.any() and bool((dq[both].abs().sum(-1) > 0).all()) and bool((dk[both].abs().sum(-1) > 0).all())
