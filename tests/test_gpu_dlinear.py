"""GPU: the fused decode-step projection (include/moka_dlinear.h, moka_amd/csrc/moka_dlinear.hip) -- base GEMV, bias and adapter term in
one launch -- against the fp64 oracle and the two-step path it replaces, its buffer contract, its contractual properties (row /
grouping independence, reproducibility), and the paths that reach it: the two PEFT mirrors, the decoder stack, a captured call -- and
the calls that must NOT reach it."""
import math
import random

import pytest
import torch

from oracle import cases as C
from oracle import moka_oracle as O
from tests.arena import Arena, Buf
from tests.decode_util import (BF, _avt_masks, _avt_module, _dev, _mirror_call, _stack, _vt_module, decode_fwd, dlinear_fwd, rel,
                               ulp_bf16_diff)
from tests.golden_util import check_inputs, golden_rel_err, load_golden

pytestmark = pytest.mark.gpu

TOL_BF16 = 1e-3            # tests/test_gpu_decode.py: a result against the oracle's value rounded to bf16
TOL_E2E = 6e-3             # tests/test_gpu_decode.py: a mirror's output against the reference golden


@pytest.fixture(autouse=True)
def _switch_on():
    """The switch ships off (functional.DLINEAR_FORWARD): every test of this file runs with it on and leaves it as it found it."""
    from moka_amd import functional as F
    saved = F.DLINEAR_FORWARD
    F.DLINEAR_FORWARD = True
    yield
    F.DLINEAR_FORWARD = saved


# ------------------------------------------------------------------------------------------ operands and the fp64 reference
BIAS_MODES = ("all", "none", "one")        # every member has a bias / none has / the LAST member alone has


class Case:
    """bf16-rounded operands (fp32 on the host), the fp64 base x W^T + bias and the oracle's y, computed once per shape and shared."""

    _cache = {}

    def __init__(self, T, d_in, d_outs, r, bias_mode, seed):
        g = torch.Generator().manual_seed(seed)
        self.T, self.d_in, self.d_outs, self.r, self.scale = T, d_in, tuple(d_outs), r, 2.0
        self.x = torch.randn(T, d_in, generator=g).to(BF).float()
        # W ~ N(0, 1) / sqrt(d_in): the base output and the adapter term are of the same size, so a missing half fails
        self.Ws = [(torch.randn(d, d_in, generator=g) / math.sqrt(d_in)).to(BF).float() for d in d_outs]
        self.As = [(torch.randn(r, d_in, generator=g) / math.sqrt(d_in)).to(BF).float() for _ in d_outs]
        self.Bs = [(torch.randn(d, r, generator=g) / math.sqrt(r)).to(BF).float() for d in d_outs]
        has = {"all": [True] * len(d_outs), "none": [False] * len(d_outs), "one": [False] * (len(d_outs) - 1) + [True]}[bias_mode]
        self.biases = [torch.randn(d, generator=g).to(BF).float() if h else None for d, h in zip(d_outs, has)]
        xd = self.x.double()
        self.base = [xd @ w.double().T + (0 if b is None else b.double()) for w, b in zip(self.Ws, self.biases)]
        self.ref = [O.plain_lora_forward(self.x, y0, a, b, self.scale) for y0, a, b in zip(self.base, self.As, self.Bs)]

    @classmethod
    def get(cls, T, d_in, d_outs, r, bias_mode):
        key = (T, d_in, tuple(d_outs), r, bias_mode)
        if key not in cls._cache:
            cls._cache.clear()                      # (one at a time: the real-width cases hold 100 MB)
            cls._cache[key] = cls(T, d_in, d_outs, r, bias_mode, seed=1000 * T + d_in + 7 * r + 13 * len(d_outs) + sum(d_outs))
        return cls._cache[key]

    def device(self, dev):
        put = lambda ts: [None if t is None else t.to(dev, BF) for t in ts]    # noqa: E731
        return self.x.to(dev, BF), put(self.Ws), put(self.biases), put(self.As), put(self.Bs)

    def run(self, dev, rows=None, members=None, T_alloc=None):
        """One launch on fresh NaN-filled outputs (a read of y would show).  rows: a slice of the tokens; members: a subset of the group."""
        x, Ws, bs, As, Bs = self.device(dev)
        m = list(range(len(self.d_outs))) if members is None else list(members)
        xs = x if rows is None else x[rows].contiguous()
        ys = [torch.full((T_alloc or xs.shape[0], self.d_outs[g]), float("nan"), dtype=BF, device=dev) for g in m]
        dlinear_fwd(xs, [Ws[g] for g in m], [bs[g] for g in m], [As[g] for g in m], [Bs[g] for g in m], ys, self.r, self.scale, T=xs.shape[0])
        return ys


# ------------------------------------------------------------------------------------------ a. oracle parity of the entry point
TS = [1, 2, 15, 16]
D_INS = [32, 96, 512, 576, 1056]         # 96: half a 64-column step; 512: one step per wave; 576: wave 0 takes two; 1056: two rounds + a half step
D_OUTS = [(32,), (96,), (160,), (96, 32, 64), (160, 160)]     # 32: fewer tiles than waves
RS = [1, 4, 8, 16, 17, 32, 33, 64]       # 1, 4: scalar B rows; 16 | 17, 32 | 33: the rank pads
SPECIAL = [
    (4, 64, (8224, 8224), 16, "one"),            # 258 blocks of 64: the column block doubles to 128, and 8224 = 64 x 128 + 32 ends in a partial block
    (16, 4096, (4096, 4096, 4096), 16, "none"),  # real widths: 7B q + k + v
    (1, 11008, (4096,), 64, "all"),              # real widths: 7B down projection, one token, rank pad 64
]


def _sweep():
    """40 seeded combinations of the axes (every listed value of every axis appears at least five times) + the three special cases."""
    rng = random.Random(20252)
    n = 40

    def axis(vals):
        out = [vals[i % len(vals)] for i in range(n)]
        rng.shuffle(out)
        return out

    Ts, dins, douts, rs, bm = axis(TS), axis(D_INS), axis(D_OUTS), axis(RS), axis(list(BIAS_MODES))
    return [(Ts[i], dins[i], douts[i], rs[i], bm[i]) for i in range(n)] + SPECIAL


SWEEP = _sweep()


def _check_sweep():
    """Checked when the module is collected: a change to the sampling that loses a listed value stops every test of this file."""
    for vals, col in ((TS, 0), (D_INS, 1), (D_OUTS, 2), (RS, 3), (BIAS_MODES, 4)):
        for v in vals:
            assert sum(1 for c in SWEEP if c[col] == v) >= 2, (col, v)
    assert sum(1 for c in SWEEP if c[4] == "one" and len(c[2]) > 1) >= 2          # a bias for one member only, in a real group
    for c in SPECIAL:
        assert c in SWEEP
    assert 40 <= len(SWEEP) <= 45


_check_sweep()


def _id(c):
    return f"T{c[0]}-in{c[1]}-out{'x'.join(map(str, c[2]))}-r{c[3]}-bias_{c[4]}"


@pytest.mark.parametrize("T,d_in,d_outs,r,bias_mode", SWEEP, ids=[_id(c) for c in SWEEP])
def test_entry_point_against_the_fp64_oracle(T, d_in, d_outs, r, bias_mode):
    """Reference: plain_lora_forward(x, x W^T + bias in fp64, A, B, scale) rounded ONCE to bf16.  Bound: the decode tests' one ulp and
    1e-3 -- fp32 accumulation over d_in <= 11008 costs ~1e-5 of a term and hi + lo 2^-17, so a single rounding stays within one ulp."""
    dev = _dev()
    cs = Case.get(T, d_in, d_outs, r, bias_mode)
    ys = cs.run(dev)
    for g, (y, ref64) in enumerate(zip(ys, cs.ref)):
        ref = ref64.to(BF)
        assert bool(torch.isfinite(y.float()).all()), f"y{g}: NaN / inf"
        e, u = rel(y, ref), ulp_bf16_diff(y, ref)
        print(f"y{g}: rel {e:.3g} ulp {u:.3g}")
        assert e <= TOL_BF16 and u <= 1.0 + 1e-6, (g, e, u)


# ------------------------------------------------------------------------------------------ b. against the two-step path
@pytest.mark.parametrize("T,d_in,d_outs,r,bias_mode", [(16, 576, (160, 160), 16, "all"), (2, 1056, (96, 32, 64), 33, "one"), (15, 512, (96,), 8, "none")])
def test_against_the_two_step_path(T, d_in, d_outs, r, bias_mode):
    """torch.nn.functional.linear + moka_decode_fwd on the same operands: the base rounded to bf16, the sum rounded again.  Measured in
    ulps at max(|y|, |base|) (the two-step path computes base + term), its two roundings are at most half an ulp each and the fused
    path's one at most half: at most 1.5 apart, and two bf16 values are a whole number of ulps apart -- unless y is below the base's
    binade, where its own ulp is the smaller: 2.  Not bit-equal by design; the fused result is the closer one to the oracle."""
    dev = _dev()
    cs = Case.get(T, d_in, d_outs, r, bias_mode)
    x, Ws, bs, As, Bs = cs.device(dev)
    fused = cs.run(dev)
    two = [torch.nn.functional.linear(x, W, b).contiguous() for W, b in zip(Ws, bs)]
    decode_fwd(x, As, Bs, two, r, cs.scale)
    err_f = err_t = 0.0
    for g in range(len(d_outs)):
        u = ulp_bf16_diff(fused[g], two[g], cs.base[g])
        print(f"y{g}: fused vs two-step {u:.3g} ulp")
        assert u <= 2.0 + 1e-6, (g, u)
        err_f += (fused[g].double().cpu() - cs.ref[g]).abs().sum().item()
        err_t += (two[g].double().cpu() - cs.ref[g]).abs().sum().item()
    print(f"summed |error|: fused {err_f:.6g}, two-step {err_t:.6g}")
    assert err_f <= err_t, (err_f, err_t)


# ------------------------------------------------------------------------------------------ c. buffer contract
@pytest.mark.parametrize("shift", [0, 16])
@pytest.mark.parametrize("bias_mode", ["all", "none"])
@pytest.mark.parametrize("T,d_in,d_outs,r", [(1, 32, (32,), 1), (15, 96, (96,), 17), (16, 160, (160, 32, 64), 8)])
def test_buffer_contract(T, d_in, d_outs, r, bias_mode, shift):
    """NaN guards around every buffer and y itself NaN before the call: the guards and the inputs are bit-identical afterwards, y is
    finite and correct for t < T -- so y was never read, and no clamped load (rows >= T, rank rows >= r, columns past d_in / d_out)
    reached a result -- and the rows >= T of a larger y allocation are untouched."""
    dev = _dev()
    cs = Case.get(T, d_in, d_outs, r, bias_mode)
    extra = 3
    spec = {"x": Buf((T, d_in), BF, "input", data=cs.x)}
    for g, d in enumerate(d_outs):
        spec[f"W{g}"] = Buf((d, d_in), BF, "input", data=cs.Ws[g])
        spec[f"A{g}"] = Buf((r, d_in), BF, "input", data=cs.As[g])
        spec[f"B{g}"] = Buf((d, r), BF, "input", data=cs.Bs[g])
        if cs.biases[g] is not None:
            spec[f"b{g}"] = Buf((d,), BF, "input", data=cs.biases[g])
        tail = torch.zeros(T + extra, d, dtype=torch.bool)
        tail[T:] = True
        spec[f"y{g}"] = Buf((T + extra, d), BF, "write", exempt=tail)
    ar = Arena(dev, spec, shift=shift, seed=T)
    G = len(d_outs)
    view = lambda n: ar.view(n) if n in spec else None    # noqa: E731
    dlinear_fwd(ar.view("x"), [view(f"W{g}") for g in range(G)], [view(f"b{g}") for g in range(G)], [view(f"A{g}") for g in range(G)],
                [view(f"B{g}") for g in range(G)], [view(f"y{g}") for g in range(G)], r, cs.scale, T=T)
    torch.cuda.synchronize()
    ar.check()
    for g in range(G):
        y = ar.view(f"y{g}")
        assert bool(torch.isfinite(y[:T].float()).all()), f"y{g}: NaN / inf"
        assert ulp_bf16_diff(y[:T], cs.ref[g].to(BF)) <= 1.0 + 1e-6
        assert torch.equal(y[T:].view(torch.int16), ar.prior(f"y{g}")[T:].view(torch.int16)), f"y{g}: rows >= T written"


# ------------------------------------------------------------------------------------------ d. bit-for-bit properties
@pytest.mark.parametrize("d_in,d_outs,r,bias_mode", [(576, (96, 32, 64), 17, "one"), (64, (8224, 8224), 16, "one")])
def test_row_grouping_and_run_independence(d_in, d_outs, r, bias_mode):
    dev = _dev()
    cs = Case.get(16, d_in, d_outs, r, bias_mode)
    full = cs.run(dev)
    again = cs.run(dev)
    for a, b in zip(full, again):                                  # two runs of the same call
        assert torch.equal(a, b)
    assert ulp_bf16_diff(full[0], cs.ref[0].to(BF)) <= 1.0 + 1e-6  # (and they are results, not two equal failures)
    for t in (0, 7, 15):                                           # a row does not depend on the other rows of its call
        one = cs.run(dev, rows=slice(t, t + 1))
        for g in range(len(d_outs)):
            assert torch.equal(one[g][0], full[g][t]), (t, g)
    for g in range(len(d_outs)):                                   # a projection does not depend on its group (8224 alone: 64-column blocks, in its group: 128)
        alone = cs.run(dev, members=(g,))
        assert torch.equal(alone[0], full[g]), g


# ------------------------------------------------------------------------------------------ e. through the mirrors
@pytest.mark.parametrize("decode_on", [False, True])
@pytest.mark.parametrize("kind,name", [("avt", "avt_decode"), ("vt", "vt_none")])
def test_mirrors_take_the_kernel_and_match_the_reference_golden(kind, name, decode_on, monkeypatch):
    from moka_amd import functional as F
    dev = _dev()
    cd = C.make_case_data(name)
    g = load_golden(name)
    check_inputs(cd, g)
    x = cd.x.to(dev, BF)
    monkeypatch.setattr(F, "DECODE_FORWARD", decode_on)          # asked first, whatever the other switch says
    linear = torch.nn.functional.linear
    calls = []
    monkeypatch.setattr(torch.nn.functional, "linear", lambda *a, **k: (calls.append(1), linear(*a, **k))[1])
    with torch.no_grad():
        mod = (_avt_module if kind == "avt" else _vt_module)(cd, dev).eval()
        n0, m0 = F.dlinear_launches, F.decode_launches
        y = _mirror_call(kind, mod, x)
        assert F.dlinear_launches == n0 + 1 and F.decode_launches == m0
    assert not calls, "the base GEMM is inside the launch: no torch.nn.functional.linear call"
    err = golden_rel_err(g, "y", y, cd.case.big)
    print(f"{name}: {err:.3g}")
    assert err < TOL_E2E


# ------------------------------------------------------------------------------------------ f. through the decoder
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

    try:
        with torch.no_grad():
            assert F.DLINEAR_FORWARD and not F.DECODE_FORWARD
            n0, m0 = F.dlinear_launches, F.decode_launches
            pre, caches = st(h[:, :S], masks)
            assert F.dlinear_launches == n0                                 # the prefill has masks: the general path
            new = decode(caches)
            assert F.dlinear_launches == n0 + 4 * len(st.layers) * steps    # q/k/v, o, gate/up, down
            F.DLINEAR_FORWARD = False
            old = decode(caches)
            st.merge_for_decode()
            merged = decode(caches)
            st.unmerge()
            assert F.dlinear_launches == n0 + 4 * len(st.layers) * steps and F.decode_launches == m0
    finally:
        F.DLINEAR_FORWARD = True
    for i in range(steps):
        e_old, e_m = rel(new[i], old[i]), rel(new[i], merged[i])
        print(f"step {i}: vs general path {e_old:.3g}, vs merged {e_m:.3g}")
        assert e_old <= 1e-2 and e_m <= 1e-2


# ------------------------------------------------------------------------------------------ g. fallbacks stay byte-for-byte
def _outcome(fn):
    """What a call gives today: its tensors, or the type of the error it raises."""
    try:
        out = fn()
    except Exception as e:            # noqa: BLE001
        return type(e)
    return out


def _same(a, b):
    if isinstance(a, type) or isinstance(b, type):
        return a is b
    return all(torch.equal(p, q) for p, q in zip(a, b)) and len(a) == len(b)


def _fallback_modules(dev):
    """name -> (module factory, call): calls the fused kernel does not serve."""
    cd = C.make_case_data("vt_none")
    cda = C.make_case_data("avt_decode")
    x17 = torch.randn(17, 1, cd.case.d_in, generator=torch.Generator().manual_seed(3)).to(dev, BF)
    x = cd.x.to(dev, BF)

    def infer(mod, inp, kind="vt"):
        with torch.no_grad():
            return (_mirror_call(kind, mod, inp),)

    def train(mod, inp):
        y = mod(inp, None, None, None)
        y.backward(cd.gy.to(dev, BF))
        return (y.detach(), mod.lora_A["text"].weight.grad, mod.lora_B["text"].weight.grad)

    def dropout(mod, inp):
        torch.manual_seed(5)
        return infer(mod, inp)

    def transposed():
        lin = _avt_module(cda, dev).eval()
        lin.weight = torch.nn.Parameter(cda.W.T.contiguous().to(dev, BF), requires_grad=False)     # stored [d_in, d_out]
        lin.fan_in_fan_out = True
        assert not lin.weight.T.is_contiguous()
        return lin

    def fp32_bias():
        m = _vt_module(cd, dev, bias=True).eval()
        base = m.get_base_layer()
        base.bias = torch.nn.Parameter(base.bias.data.float(), requires_grad=False)
        return m

    return {
        "17_tokens": (lambda: _vt_module(cd, dev).eval(), lambda m: infer(m, x17)),
        "training_call": (lambda: _vt_module(cd, dev).eval(), lambda m: train(m, x)),
        "active_dropout": (lambda: _vt_module(cd, dev, p=0.25).train(), lambda m: dropout(m, x)),
        "fan_in_fan_out": (transposed, lambda m: infer(m, cda.x.to(dev, BF), "avt")),
        "fp32_bias": (fp32_bias, lambda m: infer(m, x)),
    }


@pytest.mark.parametrize("decode_on", [False, True])
@pytest.mark.parametrize("name", ["17_tokens", "training_call", "active_dropout", "fan_in_fan_out", "fp32_bias"])
def test_fallbacks_take_todays_path_with_identical_results(name, decode_on, monkeypatch):
    from moka_amd import functional as F
    dev = _dev()
    monkeypatch.setattr(F, "DECODE_FORWARD", decode_on)
    make, call = _fallback_modules(dev)[name]
    got, moved = {}, {}
    for on in (True, False):
        monkeypatch.setattr(F, "DLINEAR_FORWARD", on)
        mod = make()
        n0, m0 = F.dlinear_launches, F.decode_launches
        got[on] = _outcome(lambda: call(mod))
        assert F.dlinear_launches == n0, name
        moved[on] = F.decode_launches - m0
    assert moved[True] == moved[False]                            # the decode kernel takes it, or not, as it does today
    assert _same(got[True], got[False]), (name, got[True] if isinstance(got[True], type) else "values differ")
    if name == "training_call":
        assert not isinstance(got[True], type) and float(got[True][1].abs().max()) > 0 and float(got[True][2].abs().max()) > 0


def test_sixteen_tokens_are_served_and_the_switch_off_moves_no_counter(monkeypatch):
    from moka_amd import functional as F
    dev = _dev()
    cd = C.make_case_data("vt_none")
    mod = _vt_module(cd, dev, bias=True).eval()                   # (a bf16 bias: served)
    x = torch.randn(17, 1, cd.case.d_in, generator=torch.Generator().manual_seed(3)).to(dev, BF)
    with torch.no_grad():
        n0, m0 = F.dlinear_launches, F.decode_launches
        y16 = mod(x[:16], None, None, None)
        assert (F.dlinear_launches, F.decode_launches) == (n0 + 1, m0)
        monkeypatch.setattr(F, "DLINEAR_FORWARD", False)
        y_off = mod(x[:16], None, None, None)
        assert (F.dlinear_launches, F.decode_launches) == (n0 + 1, m0)
    assert rel(y16, y_off) <= TOL_E2E


# ------------------------------------------------------------------------------------------ h. capturable
def test_one_call_captures_into_a_graph():
    """The entry point takes no workspace, allocates nothing and never synchronises: one call captured on one stream replays bit for
    bit on new inputs."""
    dev = _dev()
    cs = Case.get(15, 576, (96, 32, 64), 17, "one")
    x, Ws, bs, As, Bs = cs.device(dev)
    x_b = torch.randn(cs.T, cs.d_in, generator=torch.Generator().manual_seed(9)).to(dev, BF)
    static_x = x.clone()
    ys = [torch.full((cs.T, d), float("nan"), dtype=BF, device=dev) for d in cs.d_outs]
    dlinear_fwd(static_x, Ws, bs, As, Bs, ys, cs.r, cs.scale)                    # warm-up: library load
    live_a = [y.clone() for y in ys]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dlinear_fwd(static_x, Ws, bs, As, Bs, ys, cs.r, cs.scale)
    static_x.copy_(x_b)
    for y in ys:
        y.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    replayed = [y.clone() for y in ys]
    live_b = [torch.full_like(y, float("nan")) for y in ys]
    dlinear_fwd(x_b, Ws, bs, As, Bs, live_b, cs.r, cs.scale)
    for g in range(len(ys)):
        assert torch.equal(replayed[g], live_b[g]) and not torch.equal(replayed[g], live_a[g])
        assert bool(torch.isfinite(replayed[g].float()).all())
