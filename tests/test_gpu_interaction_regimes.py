"""GPU: the rank-space cross-modal softmax of moka_cross_fwd_kernel, moka_yx_kernel (the fused up-projection) and moka_cross_bwd[_keys]_kernel
at the logit regimes of tests/interaction_regimes.py -- peaked attention up to |logit| = 600, the arg-max key in every chunk position and
wave tile, waves without keys, zero key rows that hold > 99 % of the mass, logits all far below zero, query rows that are key rows --
against the fp64 oracle, with the per-sample, per-row-role bounds of tests/interaction_regimes.py (C * 2^-24 * (1 + max |logit|) * F; the
float32 emulation of the kernels' blocking passes them with at least 4x margin and every mutant of it fails them by more than 10x:
tests/test_interaction_regimes_host.py).

Every regime runs through the functional wrappers (cross_fwd, up_fwd_fused_ with want_state, cross_bwd); three regimes more run the group
forms with G = 3, each projection in a different logit regime in one launch, and must give the bits of the single-projection launches.
The last tests run the whole layer (_stage_check of tests/test_gpu_parity.py, tolerances unchanged, and the autograd node) with A scaled
so that max |logit| >= 100, the regime of trained adapters.

Observed on an MI355X (worst err / bound over every regime and projection): hp - h 0.078, dq 0.155, dK 0.086, dq + dK 0.087.

Kernel instances reached (rocprofv3 --kernel-trace --stats -- python -m pytest tests/test_gpu_interaction_regimes.py -m gpu):
moka_cross_fwd_kernel<16,4,4>, <32,4,4>, <64,2,4>; moka_cross_bwd_kernel<16|32|64>; moka_cross_bwd_keys_kernel<16|32|64>;
moka_yx_kernel<16|32|64>.
"""
import math

import pytest
import torch

from oracle import cases as C
from oracle import moka_oracle as O
from tests import interaction_regimes as IR
from tests.test_gpu_buffer_contract import _kmj_read
from tests.test_gpu_parity import TOL_E2E, _spec_and_routing, _stage_check, rel

pytestmark = pytest.mark.gpu

S_OUT = {"avt": [0.5, 2.0, 1.5], "vt": [0.75, 2.0]}
S_IN = 0.5
D_OUT = 96
REGS = IR.regimes()
GROUPS = IR.group_regimes()


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _routing(d, dev):
    from moka_amd.routing import MokaRouting
    masks = [m.to(dev) for m in d.masks]
    return MokaRouting.from_avt_masks(masks) if d.reg.variant == "avt" else MokaRouting.from_vt_masks(*masks)


def _tok_scale(d, scales):
    tm = d.rt.tok_mod[:d.T].long()
    s = torch.zeros(d.T)
    for m, v in enumerate(scales):
        s[tm == m] = v
    return s, tm


def _weights(d, dev, seed):
    g = torch.Generator().manual_seed(seed)
    Bw = (torch.randn(D_OUT, d.r, generator=g) * 0.05).to(torch.bfloat16).to(dev)
    y0 = torch.randn(d.T, D_OUT, generator=g).to(torch.bfloat16).to(dev)
    return Bw, y0


def _check_fwd(d, st, obs):
    """h to the bit, hp within its bounds, untouched rows to the bit, packs per element."""
    assert torch.equal(st.h.cpu(), d.h), "h differs from the exact sum of the slices"
    hp = st.hp.cpu()
    IR.check_forward_exact(d, hp)
    fe = IR.forward_errors(d, hp)
    obs.append(("hp-h", IR.worst(fe)))
    assert IR.worst(fe) <= 1.0, IR.fmt(fe)
    s, _ = _tok_scale(d, S_OUT[d.reg.variant])
    want = hp * s[:, None]
    RP, Tp = d.RP, st.hp_kmj.shape[-1]
    tok = st.hp_tok.float().cpu()
    assert IR.pack_error(tok[:d.T, :RP] + tok[:d.T, RP:], want) <= IR.PACK_REL, "hp_tok"
    kmj = _kmj_read(st.hp_kmj, RP, Tp)
    assert IR.pack_error(kmj[:, :d.T].t(), want) <= IR.PACK_REL, "hp_kmj"
    assert float(kmj[:, d.T:].abs().max()) == 0.0 if Tp > d.T else True


def _check_bwd(d, bst, obs):
    dh = bst.dh.cpu()
    IR.check_backward_exact(d, dh)
    be = IR.backward_errors(d, dh)
    for role in ("dq", "dK", "dq+dK"):
        rows = [x for x in be if x["role"] == role]
        if rows:
            obs.append((role, IR.worst(rows)))
    assert IR.worst(be) <= 1.0, IR.fmt(be)
    s, tm = _tok_scale(d, [S_IN] * len(S_OUT[d.reg.variant]))
    want = dh * s[:, None]
    RP, Tp = d.RP, bst.dh_kmj.shape[-1]
    tok = bst.dh_tok.float().cpu()
    assert IR.pack_error(tok[:d.T, :RP] + tok[:d.T, RP:], want) <= IR.PACK_REL, "dh_tok"
    for m in range(bst.dh_kmj.shape[0]):
        kmj = _kmj_read(bst.dh_kmj[m], RP, Tp)
        wm = torch.where((tm == m)[:, None], want, torch.zeros_like(want))
        assert IR.pack_error(kmj[:, :d.T].t(), wm) <= IR.PACK_REL, f"dh_kmj plane {m}"


def _run_single(d, dev, obs):
    from moka_amd import functional as F
    rt = _routing(d, dev)
    s_out, w, c = S_OUT[d.reg.variant], d.reg.w, d.reg.inv_sqrt_dk
    part = d.part.to(dev)
    st = F.cross_fwd(part, rt, d.r, s_out, w, c, Bw=None, want_hp=True)
    torch.cuda.synchronize()
    _check_fwd(d, st, obs)
    # the fused up-projection: the bits of cross_fwd + up_fwd
    Bw, y0 = _weights(d, dev, d.reg.seed)
    y_two = y0.clone()
    F.up_fwd_(y_two, st.hp_tok, Bw, rt, d.r)
    y_fused = y0.clone()
    fs = F.up_fwd_fused_(y_fused, part, Bw, rt, d.r, s_out, w, c, want_state=True)
    torch.cuda.synchronize()
    assert torch.equal(fs.h, st.h), "fused h"
    assert torch.equal(fs.hp_kmj, st.hp_kmj), "fused hp_kmj"
    assert torch.equal(y_fused, y_two), "fused y"
    # the backward on the kernel's own h
    bst = F.cross_bwd(d.g_part.to(dev), st.h, rt, d.r, S_IN, w, c, want_dh=True)
    torch.cuda.synchronize()
    _check_bwd(d, bst, obs)
    return rt, st, bst, (Bw, y0, y_fused)


@pytest.mark.parametrize("reg", REGS, ids=[r.id for r in REGS])
def test_interaction_regime(reg):
    d = IR.make(reg)
    obs = []
    _run_single(d, _dev(), obs)
    print(f"\n{reg.id}: max err / bound " + " ".join(f"{k}={v:.3g}" for k, v in obs))


@pytest.mark.parametrize("base,projs", GROUPS, ids=[b for b, _ in GROUPS])
def test_group_forms_run_three_regimes_in_one_launch(base, projs):
    from moka_amd import functional as F
    dev = _dev()
    ds = [IR.make(p) for p in projs]
    assert all(torch.equal(x.rt.ktok, ds[0].rt.ktok) and torch.equal(x.rt.tok_mod, ds[0].rt.tok_mod) for x in ds)
    obs = []
    singles = [_run_single(d, dev, obs) for d in ds]
    d0 = ds[0]
    rt = _routing(d0, dev)
    s_out, w, c, r = S_OUT[d0.reg.variant], d0.reg.w, d0.reg.inv_sqrt_dk, d0.r
    parts = [d.part.to(dev) for d in ds]
    Bws = [s[3][0] for s in singles]
    grp = F.cross_fwd_group(parts, rt, r, s_out, w, c, Bw=Bws)
    ys = [s[3][1].clone() for s in singles]
    fgrp = F.up_fwd_fused_group_(ys, parts, Bws, rt, r, s_out, w, c, want_state=True)
    bgrp = F.cross_bwd_group([d.g_part.to(dev) for d in ds], [s[1].h for s in singles], rt, r, S_IN, w, c)
    torch.cuda.synchronize()
    for i, (_, st, bst, (_, _, y_fused)) in enumerate(singles):
        assert torch.equal(grp[i].h, st.h) and torch.equal(grp[i].hp_kmj, st.hp_kmj) and torch.equal(grp[i].hp_tok, st.hp_tok), f"cross_fwd_group {i}"
        assert torch.equal(fgrp[i].h, st.h) and torch.equal(fgrp[i].hp_kmj, st.hp_kmj) and torch.equal(ys[i], y_fused), f"up_fwd_fused_group_ {i}"
        assert torch.equal(bgrp[i].dh_tok, bst.dh_tok) and torch.equal(bgrp[i].dh_kmj, bst.dh_kmj), f"cross_bwd_group {i}"
    print(f"\n{base} G=3 (L = {[round(max(x.L), 1) for x in ds]}): max err / bound " + " ".join(f"{k}={v:.3g}" for k, v in obs))


# ------------------------------------------------------------------------------------------------------------------------------------
# the whole layer at trained magnitude: A scaled (by a power of two: bf16 inputs stay exact) until max |logit| >= 100
# ------------------------------------------------------------------------------------------------------------------------------------
TRAINED = [
    ("trained_avt_r16", dict(variant="avt", B=2, S=301, d_in=512, d_out=384, r=16, alpha=16.0, w=1.0, seed=91,
                             layouts=[C._syn_layout(301, 64, 32, 80, 16, 16), [("p", 11)] + C._syn_layout(290, 40, 40, 70, 8, 8)])),
    ("trained_avt_r64", dict(variant="avt", B=1, S=250, d_in=256, d_out=160, r=64, alpha=16.0, w=1.0, seed=92,
                             layouts=[C._syn_layout(250, 48, 24, 70, 8, 8)])),
    ("trained_vt_r16_4096", dict(variant="vt", B=1, S=256, d_in=4096, d_out=4096, r=16, alpha=16.0, w=0.05, seed=93, big=True,
                                 layouts=[[("t", 12), ("v", 64), ("q", 30), ("I", 4), ("q", 40), ("t", 106)]])),
]


def _max_logit(cd):
    c = cd.case
    if c.variant == "avt":
        ort, s_in = O.routing_from_avt_masks(cd.masks), c.alpha / c.r
    else:
        ort, s_in = O.routing_from_vt_masks(*cd.masks), 1.0
    h = torch.zeros(c.B, c.S, c.r, dtype=torch.float64)
    for m in range(len(cd.A)):
        sel = ort.tok_mod == m
        h[sel] = s_in * (cd.x[sel].double() @ cd.A[m].double().t())
    L = 0.0
    for b in range(c.B):
        q = torch.where(ort.is_query[b])[0]
        if q.numel() and ort.kpos[b].numel():
            K = h[b, ort.kpos[b]] * ort.kvalid[b].double()[:, None]
            L = max(L, float(((h[b, q] @ K.t()) / math.sqrt(c.r)).abs().max()))
    return L


def _trained_case(name, spec):
    C._CASES[name] = spec
    cd = C.make_case_data(name)
    k = 0
    while _max_logit(cd) < 100.0:
        cd.A = [a * 2.0 for a in cd.A]
        k += 1
        assert k < 12
    assert max(len(C.build_layout(lay, spec["S"])[1].nonzero()) for lay in spec["layouts"]) > 64
    return cd


@pytest.mark.parametrize("name,spec", TRAINED, ids=[n for n, _ in TRAINED])
def test_stages_at_trained_magnitude(name, spec):
    cd = _trained_case(name, spec)
    print(f"\n{name}: max |logit| = {_max_logit(cd):.1f}")
    _stage_check(cd)


def test_autograd_node_at_trained_magnitude():
    from moka_amd.functional import moka_linear
    dev = _dev()
    name, spec = TRAINED[0]
    cd = _trained_case(name, spec)
    c = cd.case
    spec_, rt, ort = _spec_and_routing(cd, dev)
    bf = torch.bfloat16
    x = cd.x.to(dev, bf).requires_grad_(True)
    W = cd.W.to(dev, bf)
    A = [a.to(dev, bf).requires_grad_(True) for a in cd.A]
    Bw = cd.Bw.to(dev, bf).requires_grad_(True)
    y = moka_linear(x, W, None, Bw, A, rt, spec_)
    gy = cd.gy.to(dev, bf)
    y.backward(gy)
    torch.cuda.synchronize()
    T = c.B * c.S
    with torch.no_grad():       # the frozen base as the GPU computed it (bf16), the adapter terms from the fp64 oracle
        y0 = torch.nn.functional.linear(x.detach().reshape(T, -1), W).reshape(c.B, c.S, -1).double().cpu()
        dx0 = torch.matmul(gy.reshape(T, -1), W).reshape(c.B, c.S, -1).double().cpu()
    yo, ctx = O.adapter_forward(cd.x, y0, cd.A, cd.Bw, ort, spec_.s_in, spec_.s_out, spec_.w, c.r)
    dxo, dAo, dBo, _ = O.adapter_backward(cd.gy, ctx)
    assert rel(y, yo) < TOL_E2E and rel(x.grad, dxo + dx0) < TOL_E2E and rel(Bw.grad, dBo) < TOL_E2E
    for m in range(len(A)):
        assert rel(A[m].grad, dAo[m]) < TOL_E2E, m
