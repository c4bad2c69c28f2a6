"""GPU: the decode-step kernel (include/moka_decode.h, moka_amd/csrc/moka_decode.hip) against the fp64 oracle, its buffer contract, its
contractual properties (row / grouping independence, reproducibility), and the paths that reach it: the two PEFT mirrors, the
decoder stack, a captured decode step -- and the calls that must NOT reach it."""
import math
import random

import pytest
import torch

from oracle import cases as C
from oracle import moka_oracle as O
from tests.arena import Arena, Buf
from tests.decode_util import BF, _avt_masks, _avt_module, _dev, _mirror_call, _stack, _vt_module, decode_fwd, rel, ulp_bf16_diff
from tests.golden_util import check_inputs, golden_rel_err, load_golden

pytestmark = pytest.mark.gpu

TOL_BF16 = 1e-3            # tests/test_gpu_parity.py: the adapter term against the oracle's value rounded to bf16
TOL_E2E = 6e-3             # ... and with the bf16 base GEMM inside the compared value


@pytest.fixture(autouse=True)
def _switch_on():
    """The switch ships off (functional.DECODE_FORWARD): every test of this file runs with it on and leaves it as it found it."""
    from moka_amd import functional as F
    saved = F.DECODE_FORWARD
    F.DECODE_FORWARD = True
    yield
    F.DECODE_FORWARD = saved


# ------------------------------------------------------------------------------------------ a. oracle parity of the entry point
TS = [1, 2, 5, 16, 17, 33, 64]
D_INS = [32, 96, 160, 4096, 11008]
D_OUTS = [32, 96, 1024, 4096]
RS = [1, 4, 8, 16, 17, 32, 64]
GROUPS = {2: (704, 704), 3: (256, 64, 64)}


def _sweep():
    """42 seeded combinations; every listed value of every axis appears at least six times, G = 2 and G = 3 six times each."""
    rng = random.Random(20251)
    n = 42

    def axis(vals):
        out = [vals[i % len(vals)] for i in range(n)]
        rng.shuffle(out)
        return out

    Ts, dins, douts, rs = axis(TS), axis(D_INS), axis(D_OUTS), axis(RS)
    gs = [1] * (n - 12) + [2] * 6 + [3] * 6
    rng.shuffle(gs)
    return [(Ts[i], dins[i], (douts[i],) if gs[i] == 1 else GROUPS[gs[i]], rs[i]) for i in range(n)]


SWEEP = _sweep()


def _check_sweep():
    """Checked when the module is collected: a change to the sampling that loses a listed value stops every test of this file."""
    for vals, col in ((TS, 0), (D_INS, 1), (RS, 3)):
        for v in vals:
            assert sum(1 for c in SWEEP if c[col] == v) >= 2, (col, v)
    for v in D_OUTS:
        assert sum(1 for c in SWEEP if c[2] == (v,)) >= 2, v
    for g in GROUPS.values():
        assert sum(1 for c in SWEEP if c[2] == g) >= 2, g
    assert len(SWEEP) >= 40


_check_sweep()


def _operands(T, d_in, d_outs, r, seed):
    """bf16-rounded operands (fp32 on the host) and the fp64 adapter terms of the oracle."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, d_in, generator=g).to(BF).float()
    As = [(torch.randn(r, d_in, generator=g) / math.sqrt(d_in)).to(BF).float() for _ in d_outs]
    Bs = [(torch.randn(d, r, generator=g) / math.sqrt(r)).to(BF).float() for d in d_outs]
    scale = 2.0
    terms = [O.plain_lora_forward(x, torch.zeros(T, d, dtype=torch.float64), a, b, scale) for a, b, d in zip(As, Bs, d_outs)]
    # a base output of the adapter term's own size (as tests/schedule_oracle.py scales its buffers): the term is never below an ulp of it
    y0s = [(torch.randn(T, d, generator=g) * float(t.pow(2).mean().sqrt())).to(BF).float() for t, d in zip(terms, d_outs)]
    return x, As, Bs, scale, terms, y0s


@pytest.mark.parametrize("T,d_in,d_outs,r", SWEEP, ids=[f"T{c[0]}-in{c[1]}-out{'x'.join(map(str, c[2]))}-r{c[3]}" for c in SWEEP])
def test_entry_point_against_the_fp64_oracle(T, d_in, d_outs, r):
    dev = _dev()
    x, As, Bs, scale, terms, y0s = _operands(T, d_in, d_outs, r, seed=1000 * T + d_in + 7 * r + len(d_outs))
    xd, Ad, Bd = x.to(dev, BF), [a.to(dev, BF) for a in As], [b.to(dev, BF) for b in Bs]
    # the adapter term alone
    ys = [torch.zeros(T, d, dtype=BF, device=dev) for d in d_outs]
    decode_fwd(xd, Ad, Bd, ys, r, scale)
    for y, t in zip(ys, terms):
        ref = t.to(BF)
        e, u = rel(y, ref), ulp_bf16_diff(y, ref)
        print(f"term: rel {e:.3g} ulp {u:.3g}")
        assert e <= TOL_BF16 and u <= 1.0 + 1e-6, (e, u)
    # on top of a base output
    ys = [y0.to(dev, BF) for y0 in y0s]
    decode_fwd(xd, Ad, Bd, ys, r, scale)
    for y, t, y0 in zip(ys, terms, y0s):
        ref = (y0.double() + t).to(BF)
        u = ulp_bf16_diff(y, ref, y0)
        print(f"in place: ulp {u:.3g}")
        assert u <= 1.0 + 1e-6, u
        assert rel(y, ref) <= TOL_BF16


# ------------------------------------------------------------------------------------------ b. buffer contract
@pytest.mark.parametrize("shift", [0, 16])
@pytest.mark.parametrize("T,d_in,d_outs,r", [(1, 32, (32,), 1), (17, 96, (96,), 17), (64, 160, (256, 64, 64), 8)])
def test_buffer_contract(T, d_in, d_outs, r, shift):
    """Guards (NaN around the inputs) and inputs bit-identical after the call, no NaN in y: rows >= T, rank rows >= r and columns past
    d_in / d_out are never stored and never read past their buffers -- a clamped load that reached a result would carry the NaN there."""
    dev = _dev()
    x, As, Bs, scale, terms, y0s = _operands(T, d_in, d_outs, r, seed=77 + T)
    spec = {"x": Buf((T, d_in), BF, "input", data=x)}
    for g, d in enumerate(d_outs):
        spec[f"A{g}"] = Buf((r, d_in), BF, "input", data=As[g])
        spec[f"B{g}"] = Buf((d, r), BF, "input", data=Bs[g])
        spec[f"y{g}"] = Buf((T, d), BF, "inout", data=y0s[g])
    ar = Arena(dev, spec, shift=shift, seed=T)
    G = len(d_outs)
    decode_fwd(ar.view("x"), [ar.view(f"A{g}") for g in range(G)], [ar.view(f"B{g}") for g in range(G)],
               [ar.view(f"y{g}") for g in range(G)], r, scale)
    torch.cuda.synchronize()
    ar.check()
    for g in range(G):
        y = ar.view(f"y{g}")
        assert bool(torch.isfinite(y.float()).all()), f"y{g}: NaN / inf"
        ref = (y0s[g].double() + terms[g]).to(BF)
        assert ulp_bf16_diff(y, ref, y0s[g]) <= 1.0 + 1e-6
        # (a prior of the term's own size: an output that was overwritten instead of added to is off by ~1; bf16 rounding of y: 2^-9)
        ar.check_delta(f"y{g}", terms[g], 2e-2)


# ------------------------------------------------------------------------------------------ c. contractual properties
def test_row_grouping_and_run_independence():
    dev = _dev()
    T, d_in, d_outs, r = 33, 160, (256, 64, 64), 17
    x, As, Bs, scale, _, y0s = _operands(T, d_in, d_outs, r, seed=5)
    xd, Ad, Bd = x.to(dev, BF), [a.to(dev, BF) for a in As], [b.to(dev, BF) for b in Bs]

    def run(rows=None, members=(0, 1, 2)):
        xs = xd if rows is None else xd[rows].contiguous()
        ys = [(y0s[g].to(dev, BF) if rows is None else y0s[g].to(dev, BF)[rows].contiguous()) for g in members]
        decode_fwd(xs, [Ad[g] for g in members], [Bd[g] for g in members], ys, r, scale)
        return ys

    full = run()
    again = run()
    for a, b in zip(full, again):                                  # (iii) two runs of the same call
        assert torch.equal(a, b)
    for t in (0, 5, 15, 16, 31, 32):                               # (i) a row does not depend on the other rows of its call
        one = run(rows=slice(t, t + 1))
        for g in range(3):
            assert torch.equal(one[g][0], full[g][t]), (t, g)
    for g in range(3):                                             # (ii) a projection does not depend on its group
        alone = run(members=(g,))
        assert torch.equal(alone[0], full[g]), g


# ------------------------------------------------------------------------------------------ d. through the public surface
@pytest.mark.parametrize("kind,name", [("avt", "avt_decode"), ("vt", "vt_none")])
def test_mirrors_take_the_kernel_and_match_the_reference_golden(kind, name):
    from moka_amd import functional as F
    dev = _dev()
    cd = C.make_case_data(name)
    g = load_golden(name)
    check_inputs(cd, g)
    make = _avt_module if kind == "avt" else _vt_module
    x = cd.x.to(dev, BF)
    with torch.no_grad():
        mod = make(cd, dev).eval()
        n0 = F.decode_launches
        y = _mirror_call(kind, mod, x)
        assert F.decode_launches == n0 + 1
        assert golden_rel_err(g, "y", y, cd.case.big) < TOL_E2E
        # the adapter term alone (a zero base weight) against golden_y - x W^T, fp64 on the host, rounded once to bf16
        mod0 = make(cd, dev, zero_base=True).eval()
        ya = _mirror_call(kind, mod0, x)
        assert F.decode_launches == n0 + 2
    ref = torch.from_numpy(g["ref_y"]).double()
    term = (ref - (cd.x.double().reshape(-1, cd.case.d_in) @ cd.W.double().T).reshape(ref.shape)).float().to(BF)
    err = rel(ya.reshape(term.shape), term)
    print(f"{name}: adapter term rel {err:.3g}")
    assert err <= TOL_BF16, err


# ------------------------------------------------------------------------------------------ e. through the decoder
def test_decoder_steps_four_launches_per_layer():
    from moka_amd import functional as F
    dev = _dev()
    st, dims = _stack(dev)
    B, S, steps = 2, 80, 3
    masks = _avt_masks(B, S, dev)
    h = torch.randn(B, S + steps, dims.hidden, generator=torch.Generator().manual_seed(2)).to(dev, BF)

    def decode(caches):
        outs, c = [], caches
        for i in range(steps):
            o, c = st(h[:, S + i:S + i + 1], masks, kv_caches=c)
            outs.append(o)
        return outs

    saved = F.DECODE_FORWARD
    try:
        with torch.no_grad():
            F.DECODE_FORWARD = True
            n0 = F.decode_launches
            pre, caches = st(h[:, :S], masks)
            assert F.decode_launches == n0                                  # the prefill has masks: the general path
            new = decode(caches)
            assert F.decode_launches == n0 + 4 * len(st.layers) * steps     # q/k/v, o, gate/up, down
            F.DECODE_FORWARD = False
            old = decode(caches)
            assert F.decode_launches == n0 + 4 * len(st.layers) * steps
            st.merge_for_decode()
            merged = decode(caches)
            st.unmerge()
    finally:
        F.DECODE_FORWARD = saved
    for i in range(steps):
        e_old, e_m = rel(new[i], old[i]), rel(new[i], merged[i])
        print(f"step {i}: vs general path {e_old:.3g}, vs merged {e_m:.3g}")
        assert e_old <= 1e-2 and e_m <= 1e-2


# ------------------------------------------------------------------------------------------ f. fallbacks keep today's behaviour
def test_training_call_without_masks_stays_on_the_autograd_node():
    from moka_amd import functional as F
    dev = _dev()
    cd = C.make_case_data("vt_none")
    x = cd.x.to(dev, BF)
    gy = cd.gy.to(dev, BF)
    saved = F.DECODE_FORWARD
    got = {}
    try:
        for on in (True, False):
            F.DECODE_FORWARD = on
            mod = _vt_module(cd, dev).eval()
            assert mod.lora_A["text"].weight.requires_grad and mod.lora_B["text"].weight.requires_grad
            n0 = F.decode_launches
            y = mod(x, None, None, None)
            y.backward(gy)
            assert F.decode_launches == n0
            got[on] = (y.detach(), mod.lora_A["text"].weight.grad, mod.lora_B["text"].weight.grad)
    finally:
        F.DECODE_FORWARD = saved
    for a, b in zip(got[True], got[False]):
        assert a is not None and torch.equal(a, b)
    assert float(got[True][1].abs().max()) > 0 and float(got[True][2].abs().max()) > 0


def test_more_tokens_than_the_cap_stay_on_the_general_path():
    from moka_amd import functional as F
    from moka_amd.modified_peft import Linear as VtLinear       # noqa: F401
    dev = _dev()
    cd = C.make_case_data("vt_none")
    mod = _vt_module(cd, dev).eval()
    x = torch.randn(65, 1, cd.case.d_in, generator=torch.Generator().manual_seed(3)).to(dev, BF)
    saved = F.DECODE_FORWARD
    try:
        with torch.no_grad():
            F.DECODE_FORWARD = True
            n0 = F.decode_launches
            y_on = mod(x, None, None, None)
            assert F.decode_launches == n0
            y64 = mod(x[:64], None, None, None)                 # (one token fewer: the kernel)
            assert F.decode_launches == n0 + 1
            F.DECODE_FORWARD = False
            y_off = mod(x, None, None, None)
    finally:
        F.DECODE_FORWARD = saved
    assert torch.equal(y_on, y_off)
    assert rel(y64, y_off[:64]) <= TOL_E2E


def test_dropout_in_train_mode_does_not_take_the_kernel():
    from moka_amd import functional as F
    dev = _dev()
    cd = C.make_case_data("vt_none")
    mod = _vt_module(cd, dev, p=0.25)
    x = cd.x.to(dev, BF)
    with torch.no_grad():
        mod.train()
        n0 = F.decode_launches
        torch.manual_seed(5)
        y_drop = mod(x, None, None, None)
        assert F.decode_launches == n0
        mod.eval()                                              # eval() ignores lora_dropout: the kernel again
        y_eval = mod(x, None, None, None)
        assert F.decode_launches == n0 + 1
    assert not torch.equal(y_drop, y_eval)


# ------------------------------------------------------------------------------------------ g. capturable
def test_a_decode_step_captures_into_a_graph():
    """One cached decode step of the 2-layer stack (stock attention included) captured on one stream and replayed on a new input:
    the launch takes no workspace, allocates nothing and never synchronises, so the replay equals the live step bit for bit."""
    from moka_amd import functional as F
    dev = _dev()
    st, dims = _stack(dev)
    B, S = 2, 80
    masks = _avt_masks(B, S, dev)
    gen = torch.Generator().manual_seed(4)
    h = torch.randn(B, S, dims.hidden, generator=gen).to(dev, BF)
    tok_a = torch.randn(B, 1, dims.hidden, generator=gen).to(dev, BF)
    tok_b = torch.randn(B, 1, dims.hidden, generator=gen).to(dev, BF)
    assert F.DECODE_FORWARD
    with torch.no_grad():
        _, caches = st(h, masks)
        static_in = tok_a.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                           # warm-up: routing cache, library load, allocator
            for _ in range(2):
                st(static_in, masks, kv_caches=caches)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        n0 = F.decode_launches
        with torch.cuda.graph(graph):
            static_out, _ = st(static_in, masks, kv_caches=caches)
        assert F.decode_launches == n0 + 4 * len(st.layers)
        static_in.copy_(tok_b)
        graph.replay()
        torch.cuda.synchronize()
        replayed = static_out.clone()
        live, _ = st(tok_b, masks, kv_caches=caches)
        live_a, _ = st(tok_a, masks, kv_caches=caches)
    assert torch.equal(replayed, live)
    assert not torch.equal(replayed, live_a)
