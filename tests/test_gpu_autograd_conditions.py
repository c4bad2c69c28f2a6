"""The autograd node (moka_amd/functional.py: MokaLinearFn, one projection or a group of G fed by the same x) against the fp64 oracle under the conditions a
trainer creates and the other GPU files never do: partial ``requires_grad``, fp32 gradient sinks that already hold values,
non-contiguous / offset / aliased inputs and upstream gradients, trainable bias, outputs that do not reach the loss, shared parameters,
a retained graph, dropout -- and operands whose pointer is off the 16 bytes the kernels load at a time (include/moka_hip.h, "pointer
alignment").

The reference of every check is ``O.adapter_forward`` / ``O.adapter_backward`` in fp64 on the same bf16-representable inputs, plus
``x W^T`` / ``gy W`` in fp64 where a base weight is present.  Tolerances are the project's (tests/test_gpu_parity.py), not new ones:

  fp32 sinks (what the kernels added into them)                            5e-5   TOL_F32
  y / dx without a base weight, vs the oracle rounded once to bf16         1e-3   TOL_BF16, and <= 1 bf16 ulp element-wise
  bf16-cast weight gradients returned to autograd                          2e-3   (test_gpu_parity: "bf16 cast of the fp32 sum")
  fp32 storage                                                             1e-5   TOL_F32_STORAGE
  with a base weight                                                       6e-3   TOL_E2E

The 2e-3 of a bf16-cast gradient is a figure for tensors of many independent elements (one bf16 rounding is off by up to 2^-8 = 3.9e-3
of an element, ~1.5e-3 in the Frobenius norm of many).  Where the returned gradient has few independent values, or autograd itself rounds
more than once -- gbias (d_out numbers), dB under a stride-0 upstream gradient (every row the same r numbers), parameters shared by two
calls (autograd adds the two bf16 gradients in bf16) -- the oracle is rounded the way the storage format forces (class
``bf16_cast_rounded``: the oracle's fp64 value rounded to bf16 where the node or autograd rounds), and held to the same 2e-3.

Every compared figure is printed as ``FIG <class> <value> <tolerance> <what>`` before it is asserted (``pytest -s`` shows them).
"""
import functools
from ctypes import byref, c_float, c_void_p

import pytest
import torch

from oracle import cases as C
from oracle import moka_oracle as O
from tests.arena import Arena, Buf
from tests.test_gpu_parity import (TOL_BF16, TOL_E2E, TOL_F32, TOL_F32_STORAGE, _dev, _group_data, _scrambled_layout, _spec_and_routing,
                                   rel, ulp_bf16_diff)

pytestmark = pytest.mark.gpu

bf, f32 = torch.bfloat16, torch.float32
TOL_CAST = 2e-3
EINVAL = -1
NAMED = ["avt_tiny", "avt_r8", "vt_tiny", "avt_r16_q", "vt_r16_q", "avt_r64"]      # rank pads 16, 16, 16, 16, 16, 64
RP32 = "cond_rp32"                                                                 # rank pad 32 (registered on first use, as test_rank_pad_32_* does)
CASES = NAMED + [RP32]
N_MOD = {n: (2 if n.startswith("vt") else 3) for n in CASES}


def _hold(cls, what, err, tol, strict=True):
    print(f"FIG {cls} {err:.3e} {tol:g} {what}")
    assert (err < tol) if strict else (err <= tol), f"{what}: {err:.3e} (tolerance {tol:g}, class {cls})"


@functools.lru_cache(maxsize=None)
def _cd(name):
    if name == RP32 and name not in C._CASES:
        lay = _scrambled_layout(2048)
        C._CASES[name] = dict(variant="avt", B=2, S=2048, d_in=512, d_out=160, r=32, alpha=16.0, w=1.0, seed=78, big=True,
                              layouts=[lay, [("t", 3)] + lay[1:]])
    return C.make_case_data(name)


@functools.lru_cache(maxsize=None)
def _srt(name):
    """(spec, device routing, oracle routing) of a case."""
    return _spec_and_routing(_cd(name), _dev())


class Ora:
    """fp64 results of one node call: y, dx (base terms included when W / bias are given), dA_m, dB, gbias."""


def _oracle(cd, spec, ort, x=None, gy=None, W=None, bias=None, keep=None, inv_keep=1.0, A=None, Bw=None):
    c = cd.case
    x = (cd.x if x is None else x).double()
    gy = (cd.gy if gy is None else gy).double()
    A = [a.double() for a in (cd.A if A is None else A)]
    Bw = (cd.Bw if Bw is None else Bw).double()
    xm = x if keep is None else x * keep * inv_keep
    y0 = torch.zeros(c.B, c.S, Bw.shape[0], dtype=torch.float64)
    if W is not None:
        y0 = x @ W.double().t()
        if bias is not None:
            y0 = y0 + bias.double()
    yo, ctx = O.adapter_forward(xm, y0, A, Bw, ort, spec.s_in, spec.s_out, spec.w, c.r, dtype=torch.float64)
    dxm, dAo, dBo, _ = O.adapter_backward(gy, ctx)
    o = Ora()
    o.y = yo
    o.dx = dxm if keep is None else dxm * keep * inv_keep
    if W is not None:
        o.dx = o.dx + gy @ W.double()
    o.dA, o.dB = dAo, dBo
    o.gbias = gy.reshape(-1, gy.shape[-1]).sum(0)
    return o


@functools.lru_cache(maxsize=None)
def _ora_plain(name, base=False):
    cd = _cd(name)
    spec, _, ort = _srt(name)
    return _oracle(cd, spec, ort, W=cd.W if base else None)


def _pattern(like, ref):
    """A known non-zero fill of a sink, of the magnitude of the gradient it will receive (so that fp32 `pattern + gradient`
    keeps the gradient's bits to ~1e-7): 'added into' and 'overwrote' differ by the whole pattern."""
    s = float(ref.double().pow(2).mean().sqrt())
    s = s if s > 0 else 1.0
    n = like.numel()
    return (((torch.arange(n, dtype=torch.float64) % 7) - 3.5) * (s / 2)).to(f32).reshape(like.shape)


def _make_sinks(cd, ora, dev):
    pB = _pattern(cd.Bw, ora.dB).to(dev)
    pA = [_pattern(a, g).to(dev) for a, g in zip(cd.A, ora.dA)]
    return (pB.clone(), [p.clone() for p in pA]), (pB, pA)


def _check_out(tag, dt, got, want, base, operand=None):
    """y or dx of a node against the oracle at the tolerance class of (storage, base weight)."""
    if dt == f32:
        _hold("fp32_storage", tag, rel(got, want), TOL_F32_STORAGE)
    elif base:
        _hold("with_base", tag, rel(got, want), TOL_E2E)
    else:
        want_bf = want.to(bf)
        _hold("bf16_out", tag, rel(got, want_bf), TOL_BF16)
        _hold("bf16_ulp", tag + " ulp", ulp_bf16_diff(got.detach(), want_bf, operand), 1.0 + 1e-6, strict=False)


def _check_wgrad(tag, dt, grad, sink, pat, want, on, use_sinks, mult=1.0, want_rounded=None):
    """One weight gradient: through autograd (bf16 cast of the fp32 sum / fp32) or through its sink; None / untouched when not asked for.
    want_rounded: the oracle with the bf16 roundings autograd applies outside the node (module docstring), for the autograd path."""
    if use_sinks:
        assert grad is None, f"{tag}: a gradient came back through autograd although a sink is installed"
        if on:
            tol, cls = (TOL_F32, "f32_sink") if dt == bf else (TOL_F32_STORAGE, "fp32_storage")
            _hold(cls, tag + " sink", rel(sink.double() - pat.double(), mult * want), tol)
        else:
            assert torch.equal(sink, pat), f"{tag}: a sink that was not asked for changed"
    elif on:
        assert grad is not None, f"{tag}: no gradient"
        tol, cls = (TOL_CAST, "bf16_cast") if dt == bf else (TOL_F32_STORAGE, "fp32_storage")
        if want_rounded is not None:
            _hold("bf16_cast_rounded", tag, rel(grad, want_rounded), TOL_CAST)
        else:
            _hold(cls, tag, rel(grad, mult * want), tol)
    else:
        assert grad is None, f"{tag}: a gradient that was not asked for"


class _Fuse:
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        from moka_amd import functional as F
        self.prev, F.FUSE_FORWARD = F.FUSE_FORWARD, self.value

    def __exit__(self, *exc):
        from moka_amd import functional as F
        F.FUSE_FORWARD = self.prev
        return False


class _Det:
    def __enter__(self):
        from moka_amd import functional as F
        F.set_deterministic(True)

    def __exit__(self, *exc):
        from moka_amd import functional as F
        F.set_deterministic(False)
        return False


def _spec(spec0, **kw):
    from moka_amd.functional import AdapterSpec
    return AdapterSpec(spec0.r, spec0.s_in, spec0.s_out, spec0.w, spec0.inv_sqrt_dk, **kw)


# ==========================================================================================
# 1a. the requires_grad matrix
# ==========================================================================================
def _single(name, dt, x_on, B_on, A_on, use_sinks, base=False):
    """One moka_linear call + backward with the given requires_grad pattern.  Returns everything the checks need."""
    from moka_amd.functional import moka_linear
    dev = _dev()
    cd = _cd(name)
    spec0, rt, _ = _srt(name)
    ora = _ora_plain(name, base)
    x = cd.x.to(dev, dt).requires_grad_(x_on)
    Bw = cd.Bw.to(dev, dt).requires_grad_(B_on)
    A = [a.to(dev, dt).requires_grad_(on) for a, on in zip(cd.A, A_on)]
    W = cd.W.to(dev, dt) if base else None
    sinks, pats = _make_sinks(cd, ora, dev) if use_sinks else (None, None)
    y = moka_linear(x, W, None, Bw, A, rt, _spec(spec0, sinks=sinks))
    any_on = x_on or B_on or any(A_on)
    assert y.requires_grad == any_on
    if any_on:
        y.backward(cd.gy.to(dev, dt))
    torch.cuda.synchronize()
    return dict(cd=cd, ora=ora, x=x, Bw=Bw, A=A, y=y.detach(), sinks=sinks, pats=pats)


@functools.lru_cache(maxsize=None)
def _y_all_on(name, dt, fuse, base=False):
    with _Fuse(fuse):
        return _single(name, dt, True, True, (True,) * N_MOD[name], False, base)["y"]


def _check_single(tag, dt, res, x_on, B_on, A_on, use_sinks, base):
    ora = res["ora"]
    _check_out(f"{tag} y", dt, res["y"], ora.y, base)
    if x_on:
        _check_out(f"{tag} dx", dt, res["x"].grad, ora.dx, base)
    else:
        assert res["x"].grad is None
    sinks, pats = res["sinks"] or (None, [None] * 8), res["pats"] or (None, [None] * 8)
    _check_wgrad(f"{tag} dB", dt, res["Bw"].grad, sinks[0], pats[0], ora.dB, B_on, use_sinks)
    for m, on in enumerate(A_on):
        _check_wgrad(f"{tag} dA{m}", dt, res["A"][m].grad, sinks[1][m] if use_sinks else None, pats[1][m] if use_sinks else None,
                     ora.dA[m], on, use_sinks)


def _subsets(M):
    return [tuple(bool(k >> m & 1) for m in range(M)) for k in range(2 ** M)]


def _amask(A_on):
    return "A" + "".join("1" if a else "0" for a in A_on)


MATRIX = [pytest.param(n, x_on, B_on, A_on, id=f"{n}-x{int(x_on)}-B{int(B_on)}-{_amask(A_on)}")
          for n in CASES for x_on in (True, False) for B_on in (True, False) for A_on in _subsets(N_MOD[n])]


@pytest.mark.parametrize("fuse", [True, False], ids=["fused", "three_launch"])
@pytest.mark.parametrize("mode", ["grads", "sinks"])
@pytest.mark.parametrize("name,x_on,B_on,A_on", MATRIX)
def test_single_node_requires_grad_matrix_bf16(name, x_on, B_on, A_on, mode, fuse):
    """Every combination of x / lora_B / subset of lora_A_m with grad (all-off included: the output then requires no grad), through
    autograd gradients and through pre-filled fp32 sinks, with both forwards: what was asked for equals the oracle, what was not is
    None / keeps its bits, and y does not depend on the combination."""
    with _Fuse(fuse):
        res = _single(name, bf, x_on, B_on, A_on, mode == "sinks")
        _check_single(f"{name} {mode} fuse={fuse}", bf, res, x_on, B_on, A_on, mode == "sinks", False)
    assert torch.equal(res["y"], _y_all_on(name, bf, fuse)), "y depends on which inputs require grad"


@pytest.mark.parametrize("mode", ["grads", "sinks"])
@pytest.mark.parametrize("name,x_on,B_on,A_on", MATRIX)
def test_single_node_requires_grad_matrix_fp32_storage(name, x_on, B_on, A_on, mode):
    res = _single(name, f32, x_on, B_on, A_on, mode == "sinks")
    _check_single(f"{name} fp32 {mode}", f32, res, x_on, B_on, A_on, mode == "sinks", False)
    assert torch.equal(res["y"], _y_all_on(name, f32, True)), "y depends on which inputs require grad"


BASE_MATRIX = [pytest.param(n, x_on, B_on, A_on, id=f"{n}-x{int(x_on)}-B{int(B_on)}-{_amask(A_on)}")
               for n in CASES for x_on in (True, False) for B_on in (True, False)
               for A_on in ((True,) * N_MOD[n], (False,) * N_MOD[n], (False, True) + (False,) * (N_MOD[n] - 2))]


@pytest.mark.parametrize("mode", ["grads", "sinks"])
@pytest.mark.parametrize("name,x_on,B_on,A_on", BASE_MATRIX)
def test_single_node_requires_grad_matrix_with_base_weight(name, x_on, B_on, A_on, mode):
    """The same with the frozen base GEMM in front (x W^T and gy W in fp64 added to the oracle): y / dx at the end-to-end tolerance,
    the weight gradients -- which the base does not enter -- at theirs."""
    res = _single(name, bf, x_on, B_on, A_on, mode == "sinks", base=True)
    _check_single(f"{name} base {mode}", bf, res, x_on, B_on, A_on, mode == "sinks", True)
    assert torch.equal(res["y"], _y_all_on(name, bf, True, True)), "y depends on which inputs require grad"


# ---- the group node
def _group_douts(d_out, G):
    return (d_out, d_out) if G == 2 else (d_out, max(32, d_out // 2 // 32 * 32), d_out)


@functools.lru_cache(maxsize=None)
def _group(name, G):
    """(case data per projection, spec0, device routing, oracle per projection [with base]) of a G-group on the shape of a named case."""
    c = _cd(name).case
    cds = _group_data(c.variant, c.B, c.S, c.d_in, _group_douts(c.d_out, G), c.r, 9000 + c.seed, c.layouts)
    spec0, rt, ort = _spec_and_routing(cds[0], _dev())
    oras = [_oracle(cd, spec0, ort, W=cd.W) for cd in cds]
    return cds, spec0, rt, ort, oras


def _group_flags(G, M, cfg):
    """Per projection (B_on, [A_on]) of a named combination."""
    off = (False, [False] * M)
    if cfg == "all":
        return [(True, [True] * M) for _ in range(G)]
    if cfg == "B_one":                       # lora_B of ONE projection (not the first)
        return [(g == 1, [False] * M) for g in range(G)]
    if cfg == "A_one":                       # one modality of one projection (the last one's modality 1)
        return [(False, [g == G - 1 and m == 1 for m in range(M)]) for g in range(G)]
    if cfg == "one_all":                     # everything of the first projection, nothing of the others
        return [(True, [True] * M) if g == 0 else off for g in range(G)]
    raise ValueError(cfg)


def _run_group(name, G, x_on, flags, use_sinks, dt=bf, bias_on=None, gy_none=(), p=0.0):
    from moka_amd.functional import moka_linear_group
    dev = _dev()
    cds, spec0, rt, _, oras = _group(name, G)
    x = cds[0].x.to(dev, dt).requires_grad_(x_on)
    projs, sinks, pats, specs = [], [], [], []
    for g, cd in enumerate(cds):
        B_on, A_on = flags[g]
        b = None
        if bias_on is not None:
            b = (torch.arange(cd.W.shape[0], dtype=torch.float32) % 5 - 2).mul(0.125).to(dev, dt).requires_grad_(bias_on[g])
        projs.append((cd.W.to(dev, dt), b, cd.Bw.to(dev, dt).requires_grad_(B_on), [a.to(dev, dt).requires_grad_(on) for a, on in zip(cd.A, A_on)]))
        sk, pt = _make_sinks(cd, oras[g], dev) if use_sinks else (None, None)
        sinks.append(sk)
        pats.append(pt)
        specs.append(_spec(spec0, sinks=sk, dropout_p=p, seed=4711 + 13 * g))
    ys = moka_linear_group(x, projs, rt, specs)
    live = [g for g in range(G) if g not in gy_none]
    if ys[0].requires_grad:
        torch.autograd.backward([ys[g] for g in live], [cds[g].gy.to(dev, dt) for g in live])
    torch.cuda.synchronize()
    return dict(x=x, projs=projs, ys=[y.detach() for y in ys], sinks=sinks, pats=pats, specs=specs)


@functools.lru_cache(maxsize=None)
def _group_y_all_on(name, G, fuse):
    with _Fuse(fuse):
        return _run_group(name, G, True, _group_flags(G, N_MOD[name], "all"), False)["ys"]


def _check_group(tag, name, G, res, x_on, flags, use_sinks, gy_none=()):
    cds, _, _, _, oras = _group(name, G)
    for g in range(G):
        _check_out(f"{tag} y[{g}]", bf, res["ys"][g], oras[g].y, True)
    if x_on:
        _check_out(f"{tag} dx", bf, res["x"].grad, sum(oras[g].dx for g in range(G) if g not in gy_none), True)
    else:
        assert res["x"].grad is None
    for g in range(G):
        B_on, A_on = flags[g]
        mult = 0.0 if g in gy_none else 1.0
        sk, pt = (res["sinks"][g], res["pats"][g]) if use_sinks else ((None, [None] * 8), (None, [None] * 8))
        if mult == 0.0:                                            # an output that did not reach the loss: exact zeros
            if use_sinks:
                assert torch.equal(sk[0], pt[0]) and all(torch.equal(a, b) for a, b in zip(sk[1], pt[1])), f"{tag}: sinks of the unused output {g} changed"
            else:
                for t_, on in [(res["projs"][g][2], B_on)] + list(zip(res["projs"][g][3], A_on)):
                    assert (t_.grad is None) if not on else (float(t_.grad.abs().max()) == 0.0), f"{tag}: gradient of the unused output {g}"
            continue
        _check_wgrad(f"{tag} dB[{g}]", bf, res["projs"][g][2].grad, sk[0], pt[0], oras[g].dB, B_on, use_sinks)
        for m, on in enumerate(A_on):
            _check_wgrad(f"{tag} dA[{g}][{m}]", bf, res["projs"][g][3][m].grad, sk[1][m], pt[1][m], oras[g].dA[m], on, use_sinks)


@pytest.mark.parametrize("fuse", [True, False], ids=["fused", "three_launch"])
@pytest.mark.parametrize("mode", ["grads", "sinks"])
@pytest.mark.parametrize("cfg", ["B_one", "A_one", "one_all"])
@pytest.mark.parametrize("x_on", [True, False], ids=["x1", "x0"])
@pytest.mark.parametrize("G", [2, 3])
@pytest.mark.parametrize("name", CASES)
def test_group_node_requires_grad_matrix(name, G, x_on, cfg, mode, fuse):
    """MokaLinearFn on a group with gradients asked of ONE lora_B, of ONE lora_A_m, or of one whole projection only (x on and off): the
    accumulators are carved out of one flat buffer by what is needed, so every slice has to land on its own parameter."""
    flags = _group_flags(G, N_MOD[name], cfg)
    with _Fuse(fuse):
        res = _run_group(name, G, x_on, flags, mode == "sinks")
        _check_group(f"{name} G={G} {cfg} {mode} fuse={fuse}", name, G, res, x_on, flags, mode == "sinks")
    for a_, b_ in zip(res["ys"], _group_y_all_on(name, G, fuse)):
        assert torch.equal(a_, b_), "y depends on which inputs require grad"


@pytest.mark.parametrize("name", CASES)
def test_all_off_gives_an_output_without_grad(name):
    """Nothing requires grad: no error, outputs with requires_grad == False, the same bits -- single node (both storages) and group."""
    for dt in (bf, f32):
        res = _single(name, dt, False, False, (False,) * N_MOD[name], False)
        assert not res["y"].requires_grad and torch.equal(res["y"], _y_all_on(name, dt, True))
    flags = [(False, [False] * N_MOD[name])] * 3
    from moka_amd.functional import moka_linear_group
    cds, spec0, rt, _, _ = _group(name, 3)
    dev = _dev()
    ys = moka_linear_group(cds[0].x.to(dev, bf), [(cd.W.to(dev, bf), None, cd.Bw.to(dev, bf), [a.to(dev, bf) for a in cd.A]) for cd in cds],
                           rt, [_spec(spec0) for _ in cds])
    assert not any(y.requires_grad for y in ys) and len(flags) == 3
    for a_, b_ in zip(ys, _group_y_all_on(name, 3, True)):
        assert torch.equal(a_, b_)


# ==========================================================================================
# 1b. layout and aliasing of the inputs
# ==========================================================================================
def _leaf(t, dev, dt=bf):
    return t.to(dev, dt).clone().requires_grad_(True)


def _layout_run(name, make_x, loss_of, base=True, sinks=False, flat_params=None, p=0.0, seed=0):
    """One single-node call on inputs built by `make_x(dense x) -> (leaf, view fed to the node)`, a loss built by `loss_of(y, gy)`,
    parameters either plain leaves or views (`flat_params`: 'transposed' | 'flat').  Returns (y, dx on the leaf's view, dB, [dA_m])."""
    from moka_amd.functional import moka_linear
    dev = _dev()
    cd = _cd(name)
    spec0, rt, _ = _srt(name)
    leaf, x = make_x(cd.x.to(dev, bf))
    W = cd.W.to(dev, bf) if base else None
    M = len(cd.A)
    if flat_params == "transposed":
        leaves = [_leaf(cd.Bw.t().contiguous(), dev)] + [_leaf(a.t().contiguous(), dev) for a in cd.A]
        Bw, A = leaves[0].t(), [l_.t() for l_ in leaves[1:]]
        grads = lambda: (leaves[0].grad.t(), [l_.grad.t() for l_ in leaves[1:]])                        # noqa: E731
    elif flat_params == "flat":
        # ONE packed parameter buffer (what attach()'s working copy is), every parameter a view at a 16-byte aligned offset
        ts = [cd.Bw] + list(cd.A)
        offs, off = [], 8
        for t_ in ts:
            offs.append(off)
            off += (t_.numel() + 7) // 8 * 8
        flat = torch.zeros(off, dtype=bf, device=dev)
        for t_, o_ in zip(ts, offs):
            flat[o_:o_ + t_.numel()] = t_.to(dev, bf).reshape(-1)
        flat.requires_grad_(True)
        vs = [flat[o_:o_ + t_.numel()].view(t_.shape) for t_, o_ in zip(ts, offs)]
        Bw, A = vs[0], vs[1:]
        grads = lambda: (flat.grad[offs[0]:offs[0] + ts[0].numel()].view(ts[0].shape),                  # noqa: E731
                         [flat.grad[o_:o_ + t_.numel()].view(t_.shape) for t_, o_ in zip(ts[1:], offs[1:])])
    else:
        Bw, A = _leaf(cd.Bw, dev), [_leaf(a, dev) for a in cd.A]
        grads = lambda: (Bw.grad, [a.grad for a in A])                                                  # noqa: E731
    ora0 = _ora_plain(name, base)
    sk, pt = _make_sinks(cd, ora0, dev) if sinks else (None, None)
    y = moka_linear(x, W, None, Bw, A, rt, _spec(spec0, sinks=sk, dropout_p=p, seed=seed))
    loss_of(y, cd.gy.to(dev, bf))
    torch.cuda.synchronize()
    dB, dA = grads() if not sinks else (None, [None] * M)
    return dict(y=y.detach(), leaf=leaf, dx=leaf.grad, dB=dB, dA=dA, sinks=sk, pats=pt)


def _dense_x(x):
    leaf = x.clone().requires_grad_(True)
    return leaf, leaf


def _plain_loss(y, gy):
    y.backward(gy)


def _same_bits(tag, a, b):
    for k in ("y", "dx", "dB"):
        if a[k] is not None or b[k] is not None:
            assert torch.equal(a[k], b[k]), f"{tag}: {k} differs from the run on contiguous copies"
    for m, (ga, gb) in enumerate(zip(a["dA"], b["dA"])):
        if ga is not None or gb is not None:
            assert torch.equal(ga, gb), f"{tag}: dA{m} differs from the run on contiguous copies"
    if a["sinks"] is not None:
        assert torch.equal(a["sinks"][0], b["sinks"][0]) and all(torch.equal(s_, t_) for s_, t_ in zip(a["sinks"][1], b["sinks"][1])), f"{tag}: sinks differ"


def _check_layout(tag, res, ora, base=True, dx=None, few_dB_values=False):
    """few_dB_values: a stride-0 upstream gradient makes every row of dB the same r numbers (module docstring)."""
    _check_out(f"{tag} y", bf, res["y"], ora.y, base)
    _check_out(f"{tag} dx", bf, res["dx"] if dx is None else dx, ora.dx, base)
    if res["sinks"] is None:
        if few_dB_values:
            _hold("bf16_cast_rounded", f"{tag} dB", rel(res["dB"], ora.dB.to(bf)), TOL_CAST)
        else:
            _hold("bf16_cast", f"{tag} dB", rel(res["dB"], ora.dB), TOL_CAST)
        for m in range(len(ora.dA)):
            _hold("bf16_cast", f"{tag} dA{m}", rel(res["dA"][m], ora.dA[m]), TOL_CAST)
    else:
        _hold("f32_sink", f"{tag} dB sink", rel(res["sinks"][0].double() - res["pats"][0].double(), ora.dB), TOL_F32)
        for m in range(len(ora.dA)):
            _hold("f32_sink", f"{tag} dA{m} sink", rel(res["sinks"][1][m].double() - res["pats"][1][m].double(), ora.dA[m]), TOL_F32)


def _x_wide(x):
    """x as columns 32 .. 32 + d_in of a wider buffer: row pitch > d_in."""
    B, S, d = x.shape
    wide = torch.full((B, S, d + 64), 7.0, dtype=x.dtype, device=x.device)
    wide[..., 32:32 + d] = x
    wide.requires_grad_(True)
    return wide, wide[..., 32:32 + d]


def _x_transposed(x):
    leaf = x.transpose(0, 1).contiguous().requires_grad_(True)           # [S, B, d]
    return leaf, leaf.transpose(0, 1)


def _x_offset(x):
    """x contiguous at a non-zero, 16-byte aligned storage offset (8 bf16 elements)."""
    flat = torch.zeros(x.numel() + 8, dtype=x.dtype, device=x.device)
    flat[8:] = x.reshape(-1)
    flat.requires_grad_(True)
    v = flat[8:].view(x.shape)
    assert v.storage_offset() == 8 and v.is_contiguous() and v.data_ptr() % 16 == 0
    return flat, v


def _dx_of(kind, res, shape):
    g = res["dx"]
    if kind == "wide":
        d = shape[-1]
        assert float(g[..., :32].abs().max()) == 0.0 and float(g[..., 32 + d:].abs().max()) == 0.0, "gradient outside the slice"
        return g[..., 32:32 + d]
    if kind == "transposed":
        return g.transpose(0, 1)
    if kind == "offset":
        assert float(g[:8].abs().max()) == 0.0
        return g[8:].view(shape)
    return g


@pytest.mark.parametrize("kind", ["wide", "transposed", "offset"])
@pytest.mark.parametrize("name", CASES)
def test_x_views_equal_their_contiguous_copies_and_the_oracle(name, kind):
    make = {"wide": _x_wide, "transposed": _x_transposed, "offset": _x_offset}[kind]
    with _Det():
        a = _layout_run(name, make, _plain_loss)
        b = _layout_run(name, _dense_x, _plain_loss)
    a["dx"] = _dx_of(kind, a, b["dx"].shape)
    _same_bits(f"{name} x {kind}", a, b)
    _check_layout(f"{name} x {kind}", a, _ora_plain(name, True))


def _heads(d_out):
    return 4 if d_out % 4 == 0 else 1


def _loss_head_split(y, gy):
    """The loss sees y as attention heads: view(B, S, H, D).transpose(1, 2) -- the upstream gradient of q / k / v in every block."""
    B, S, d = y.shape
    H = _heads(d)
    w = gy.view(B, S, H, d // H).transpose(1, 2).contiguous()            # [B, H, S, D]: what multiplies the head-major activations
    (y.view(B, S, H, d // H).transpose(1, 2) * w).sum().backward()


def _loss_cat_slice(y, gy):
    """y is concatenated with another tensor before the loss: autograd hands the node a SLICE of the wider gradient (row pitch > d_out,
    storage larger than the view)."""
    B, S, d = y.shape
    other = torch.ones(B, S, 32, dtype=y.dtype, device=y.device)
    w = torch.cat([gy, other], dim=-1)
    (torch.cat([y, other], dim=-1) * w).sum().backward()


def _loss_sum(y, gy):
    y.sum().backward()                                                    # the gradient is a stride-0 expand of one element


@pytest.mark.parametrize("kind", ["head_split", "cat_slice", "sum"])
@pytest.mark.parametrize("name", CASES)
def test_upstream_gradient_layouts_equal_their_contiguous_copies_and_the_oracle(name, kind):
    loss = {"head_split": _loss_head_split, "cat_slice": _loss_cat_slice, "sum": _loss_sum}[kind]
    cd = _cd(name)
    spec, _, ort = _srt(name)
    gy_eff = torch.ones_like(cd.gy) if kind == "sum" else cd.gy
    dev = _dev()
    with _Det():
        a = _layout_run(name, _dense_x, loss)
        b = _layout_run(name, _dense_x, lambda y, gy: y.backward(gy_eff.to(dev, bf).contiguous()))
    _same_bits(f"{name} gy {kind}", a, b)
    _check_layout(f"{name} gy {kind}", a, _oracle(cd, spec, ort, gy=gy_eff, W=cd.W), few_dB_values=kind == "sum")


@pytest.mark.parametrize("kind", ["transposed", "flat"])
@pytest.mark.parametrize("name", CASES)
def test_parameter_views_equal_their_contiguous_copies_and_the_oracle(name, kind):
    """lora_A_m / lora_B as transposed views of [d_in, r] / [r, d_out] leaves, and as views into ONE flat parameter buffer."""
    with _Det():
        a = _layout_run(name, _dense_x, _plain_loss, flat_params=kind)
        b = _layout_run(name, _dense_x, _plain_loss)
    _same_bits(f"{name} params {kind}", a, b)
    _check_layout(f"{name} params {kind}", a, _ora_plain(name, True))


@pytest.mark.parametrize("name", CASES)
def test_group_with_an_output_that_does_not_reach_the_loss(name):
    """gys[g] is None for one member: its weight gradients are exact zeros (sinks: untouched), dx is the sum over the others."""
    G, M = 3, N_MOD[name]
    flags = _group_flags(G, M, "all")
    for use_sinks in (False, True):
        res = _run_group(name, G, True, flags, use_sinks, gy_none=(1,))
        _check_group(f"{name} G=3 unused output sinks={use_sinks}", name, G, res, True, flags, use_sinks, gy_none=(1,))


@pytest.mark.parametrize("name", CASES)
def test_trainable_bias_single_node_and_one_group_member(name):
    """gbias against the fp64 column sum of gy: the single node (with its base weight), and ONE member of a group only."""
    from moka_amd.functional import moka_linear
    dev = _dev()
    cd = _cd(name)
    spec0, rt, ort = _srt(name)
    bias = (torch.arange(cd.case.d_out, dtype=torch.float32) % 5 - 2).mul(0.125)
    b = bias.to(dev, bf).requires_grad_(True)
    x, Bw, A = _leaf(cd.x, dev), _leaf(cd.Bw, dev), [_leaf(a, dev) for a in cd.A]
    y = moka_linear(x, cd.W.to(dev, bf), b, Bw, A, rt, _spec(spec0))
    y.backward(cd.gy.to(dev, bf))
    ora = _oracle(cd, spec0, ort, W=cd.W, bias=bias)
    _check_out(f"{name} bias y", bf, y.detach(), ora.y, True)
    _check_out(f"{name} bias dx", bf, x.grad, ora.dx, True)
    _hold("bf16_cast_rounded", f"{name} gbias", rel(b.grad, ora.gbias.to(bf)), TOL_CAST)
    _hold("bf16_cast", f"{name} bias dB", rel(Bw.grad, ora.dB), TOL_CAST)
    # one group member only
    G = 3
    res = _run_group(name, G, True, _group_flags(G, N_MOD[name], "all"), False, bias_on=[False, True, False])
    cds, _, _, _, oras = _group(name, G)
    for g in range(G):
        gb = res["projs"][g][1].grad
        if g == 1:
            _hold("bf16_cast_rounded", f"{name} group gbias[{g}]", rel(gb, oras[g].gbias.to(bf)), TOL_CAST)
        else:
            assert gb is None
        bias_g = res["projs"][g][1].detach().double().cpu()
        _check_out(f"{name} group bias y[{g}]", bf, res["ys"][g], oras[g].y + bias_g, True)


@pytest.mark.parametrize("use_sinks", [False, True], ids=["grads", "sinks"])
@pytest.mark.parametrize("name", CASES)
def test_parameters_shared_by_two_calls_in_one_graph(name, use_sinks):
    """The same lora_A_m / lora_B in two node calls (two inputs), one backward: the gradients are the sum of the two oracle gradients;
    with sinks both calls accumulate into them."""
    from moka_amd.functional import moka_linear
    dev = _dev()
    cd = _cd(name)
    spec0, rt, ort = _srt(name)
    x2_, gy2_ = cd.x.flip(-1) * 0.5, cd.gy.flip(-1) * -0.5               # (still bf16-representable)
    o1, o2 = _ora_plain(name, False), _oracle(cd, spec0, ort, x=x2_, gy=gy2_)
    want = Ora()
    want.dB, want.dA = o1.dB + o2.dB, [a + b for a, b in zip(o1.dA, o2.dA)]
    sk, pt = _make_sinks(cd, want, dev) if use_sinks else (None, None)
    Bw, A = _leaf(cd.Bw, dev), [_leaf(a, dev) for a in cd.A]
    xa, xb = _leaf(cd.x, dev), _leaf(x2_, dev)
    spec = _spec(spec0, sinks=sk)
    ya, yb = moka_linear(xa, None, None, Bw, A, rt, spec), moka_linear(xb, None, None, Bw, A, rt, spec)
    torch.autograd.backward([ya, yb], [cd.gy.to(dev, bf), gy2_.to(dev, bf)])
    torch.cuda.synchronize()
    _check_out(f"{name} shared dx a", bf, xa.grad, o1.dx, False)
    _check_out(f"{name} shared dx b", bf, xb.grad, o2.dx, False)
    # through autograd each call returns its gradient rounded to bf16 and the engine adds the two in bf16: the oracle's sum with those
    # three roundings; through the sinks both calls add fp32 into the same buffer: the fp64 sum
    two = lambda a, b: (a.to(bf) + b.to(bf)).double()                  # noqa: E731
    _check_wgrad(f"{name} shared dB", bf, Bw.grad, sk[0] if sk else None, pt[0] if pt else None, want.dB, True, use_sinks,
                 want_rounded=two(o1.dB, o2.dB))
    for m in range(len(A)):
        _check_wgrad(f"{name} shared dA{m}", bf, A[m].grad, sk[1][m] if sk else None, pt[1][m] if pt else None, want.dA[m], True, use_sinks,
                     want_rounded=two(o1.dA[m], o2.dA[m]))


@pytest.mark.parametrize("use_sinks", [False, True], ids=["grads", "sinks"])
@pytest.mark.parametrize("name", CASES)
def test_backward_twice_on_a_retained_graph_doubles(name, use_sinks):
    from moka_amd.functional import moka_linear
    dev = _dev()
    cd = _cd(name)
    spec0, rt, _ = _srt(name)
    ora = _ora_plain(name, False)
    sk, pt = _make_sinks(cd, ora, dev) if use_sinks else (None, None)
    x, Bw, A = _leaf(cd.x, dev), _leaf(cd.Bw, dev), [_leaf(a, dev) for a in cd.A]
    y = moka_linear(x, None, None, Bw, A, rt, _spec(spec0, sinks=sk))
    gy = cd.gy.to(dev, bf)
    y.backward(gy, retain_graph=True)
    y.backward(gy)
    torch.cuda.synchronize()
    # x.grad is the bf16 sum of two equal bf16 gradients: exactly twice one of them
    _check_out(f"{name} twice dx", bf, x.grad, 2 * ora.dx, False)
    _check_wgrad(f"{name} twice dB", bf, Bw.grad, sk[0] if sk else None, pt[0] if pt else None, ora.dB, True, use_sinks, mult=2.0)
    for m in range(len(A)):
        _check_wgrad(f"{name} twice dA{m}", bf, A[m].grad, sk[1][m] if sk else None, pt[1][m] if pt else None, ora.dA[m], True, use_sinks, mult=2.0)


def _keep(p, seed, cd, d_in=None):
    from moka_amd import _lib
    from moka_amd import functional as F
    c = cd.case
    keep = F.dropout_mask(p, seed, c.B * c.S, c.d_in, _dev()).cpu().double().reshape(c.B, c.S, c.d_in)
    return keep, float(_lib.load().moka_dropout_scale(p))


@pytest.mark.parametrize("name", CASES)
def test_dropout_under_partial_grads_views_and_a_group(name):
    """lora_dropout > 0 on one condition of each block, replayed through moka_dropout_mask and the oracle: (a) x without grad, one
    lora_A_m and lora_B through sinks; (b) transposed x with a stride-0 upstream gradient; (c) a group with gradients of one projection."""
    from moka_amd.functional import moka_linear
    dev = _dev()
    cd = _cd(name)
    M = len(cd.A)
    spec0, rt, ort = _srt(name)
    p, seed = 0.1, 0x5eed0 + cd.case.seed
    keep, inv_keep = _keep(p, seed, cd)
    # (a)
    ora = _oracle(cd, spec0, ort, keep=keep, inv_keep=inv_keep)
    A_on = tuple(m == M - 1 for m in range(M))
    sk, pt = _make_sinks(cd, ora, dev)
    x = cd.x.to(dev, bf)
    Bw, A = _leaf(cd.Bw, dev), [a.to(dev, bf).requires_grad_(on) for a, on in zip(cd.A, A_on)]
    y = moka_linear(x, None, None, Bw, A, rt, _spec(spec0, sinks=sk, dropout_p=p, seed=seed))
    y.backward(cd.gy.to(dev, bf))
    torch.cuda.synchronize()
    _check_out(f"{name} dropout(a) y", bf, y.detach(), ora.y, False)
    _check_wgrad(f"{name} dropout(a) dB", bf, Bw.grad, sk[0], pt[0], ora.dB, True, True)
    for m in range(M):
        _check_wgrad(f"{name} dropout(a) dA{m}", bf, A[m].grad, sk[1][m], pt[1][m], ora.dA[m], A_on[m], True)
    # (b)
    ones = torch.ones_like(cd.gy)
    ora_b = _oracle(cd, spec0, ort, gy=ones, W=cd.W, keep=keep, inv_keep=inv_keep)
    res = _layout_run(name, _x_transposed, _loss_sum, p=p, seed=seed)
    res["dx"] = res["dx"].transpose(0, 1)
    _check_layout(f"{name} dropout(b)", res, ora_b, few_dB_values=True)
    # (c)
    G = 2
    cds, _, _, _, _ = _group(name, G)
    flags = _group_flags(G, M, "one_all")
    res = _run_group(name, G, True, flags, False, p=p)
    oras = []
    for g in range(G):
        kg, ik = _keep(p, res["specs"][g].seed, cds[g])
        oras.append(_oracle(cds[g], spec0, ort, W=cds[g].W, keep=kg, inv_keep=ik))
    for g in range(G):
        _check_out(f"{name} dropout(c) y[{g}]", bf, res["ys"][g], oras[g].y, True)
    _check_out(f"{name} dropout(c) dx", bf, res["x"].grad, sum(o.dx for o in oras), True)
    _hold("bf16_cast", f"{name} dropout(c) dB[0]", rel(res["projs"][0][2].grad, oras[0].dB), TOL_CAST)
    for m in range(M):
        _hold("bf16_cast", f"{name} dropout(c) dA[0][{m}]", rel(res["projs"][0][3][m].grad, oras[0].dA[m]), TOL_CAST)
    assert res["projs"][1][2].grad is None and all(a.grad is None for a in res["projs"][1][3])


# ==========================================================================================
# 1c. pointer alignment
# ==========================================================================================
def _odd_view(t, dev, dt, shift):
    """A contiguous copy of `t` that starts `shift` elements into a packed buffer (data_ptr off the 16-byte boundary)."""
    flat = torch.zeros(t.numel() + 16, dtype=dt, device=dev)
    flat[shift:shift + t.numel()] = t.to(dev, dt).reshape(-1)
    v = flat[shift:shift + t.numel()].view(t.shape)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


@pytest.mark.parametrize("which", ["x", "gy", "A", "Bw", "all"])
@pytest.mark.parametrize("name", CASES)
def test_moka_linear_on_misaligned_views_gives_the_oracles_answer(name, which):
    """A CONTIGUOUS x / gy / lora_A_m / lora_B whose data_ptr() is not a multiple of 16 (an odd element offset of a packed buffer): the
    wrappers copy it as they copy a strided view -- the library would refuse it -- and the results are those of the aligned call, bit
    for bit under deterministic weight gradients."""
    from moka_amd.functional import moka_linear
    dev = _dev()
    cd = _cd(name)
    spec0, rt, _ = _srt(name)
    ora = _ora_plain(name, True)
    W = cd.W.to(dev, bf)

    def run(mis):
        pick = lambda k, t, sh: (_odd_view(t, dev, bf, sh) if mis and which in (k, "all") else t.to(dev, bf).clone())     # noqa: E731
        x = pick("x", cd.x, 1).requires_grad_(True)
        Bw = pick("Bw", cd.Bw, 3).requires_grad_(True)
        A = [pick("A", a, 1 + 2 * m).requires_grad_(True) for m, a in enumerate(cd.A)]
        gy = pick("gy", cd.gy, 5)
        y = moka_linear(x, W, None, Bw, A, rt, _spec(spec0))
        y.backward(gy)
        torch.cuda.synchronize()
        return dict(y=y.detach(), dx=x.grad, dB=Bw.grad, dA=[a.grad for a in A], sinks=None, pats=None)

    with _Det():
        a, b = run(True), run(False)
    _same_bits(f"{name} misaligned {which}", a, b)
    _check_layout(f"{name} misaligned {which}", a, ora)


@pytest.mark.parametrize("name", CASES)
def test_fp32_sinks_at_an_odd_element_offset_are_accumulated_in_place(name):
    """The gradient sinks are the one operand that needs no 16 bytes (fp32 atomics / dword read-modify-write, include/moka_hip.h): views
    one float past a 16-byte boundary are used as they are -- no copy could be: the kernels add INTO them -- with atomics and in the
    deterministic mode."""
    from moka_amd.functional import moka_linear
    dev = _dev()
    cd = _cd(name)
    spec0, rt, _ = _srt(name)
    ora = _ora_plain(name, False)
    for det in (False, True):
        pB = _odd_view(_pattern(cd.Bw, ora.dB), dev, f32, 1)
        pA = [_odd_view(_pattern(a, g), dev, f32, 1 + (m % 3)) for m, (a, g) in enumerate(zip(cd.A, ora.dA))]
        sk, pt = (pB, pA), (pB.clone(), [t.clone() for t in pA])
        x, Bw, A = _leaf(cd.x, dev), _leaf(cd.Bw, dev), [_leaf(a, dev) for a in cd.A]
        ctx = _Det() if det else _Fuse(True)
        with ctx:
            y = moka_linear(x, None, None, Bw, A, rt, _spec(spec0, sinks=sk))
            y.backward(cd.gy.to(dev, bf))
            torch.cuda.synchronize()
        _check_wgrad(f"{name} odd sink det={det} dB", bf, Bw.grad, sk[0], pt[0], ora.dB, True, True)
        for m in range(len(A)):
            _check_wgrad(f"{name} odd sink det={det} dA{m}", bf, A[m].grad, sk[1][m], pt[1][m], ora.dA[m], True, True)


# ---- through the C ABI: a misaligned pointer is refused before anything is launched
def _abi_setup():
    """Shapes and a routing for the refusal calls (nothing is ever launched with them: the call must return MOKA_EINVAL first)."""
    from moka_amd import _lib as L
    cd = _cd("avt_r8")
    c = cd.case
    spec, rt, _ = _srt("avt_r8")
    T, RP, Tp = c.B * c.S, L.rank_pad(c.r), L.tok_pad(c.B * c.S)
    return L, L.load(), cd, c, spec, rt, T, RP, Tp


def _stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def _vp(ptrs):
    return (c_void_p * len(ptrs))(*ptrs)


def _fl(vals):
    return (c_float * len(vals))(*[float(v) for v in vals])


def _abi_calls():
    """entry point -> (arena spec, call(arena, ptr) -> rc, operands with their required alignment).  `ptr(name)` is the arena pointer of
    the buffer, moved off its requirement for the operand under test."""
    L, lib, cd, c, spec, rt, T, RP, Tp = _abi_setup()
    M, r, d_in, d_out = len(cd.A), c.r, c.d_in, c.d_out
    ks, ksb = L.ksplit(T, d_in, r), L.ksplit_bwd(T, d_out, r)
    z = lambda *shape: torch.zeros(*shape)                                                             # noqa: E731
    inp = lambda shape, dt=bf: Buf(shape, dt, "input", data=z(*shape))                                 # noqa: E731
    out = lambda shape, dt=bf: Buf(shape, dt, "write")                                                 # noqa: E731
    io = lambda shape, dt=bf: Buf(shape, dt, "inout", data=z(*shape))                                  # noqa: E731
    s_out = _fl(spec.s_out)
    calls = {}
    calls["moka_down_fwd"] = (
        dict(x=inp((T, d_in)), **{f"A{m}": inp((r, d_in)) for m in range(M)}, part=out((ks, T, RP), f32)),
        lambda p: lib.moka_down_fwd(p("x"), _vp([p(f"A{m}") for m in range(M)]), rt.tok_mod.data_ptr(), p("part"), T, d_in, r, M,
                                    spec.s_in, 0.0, 0, L.MOKA_BF16, None, _stream()),
        {"x": 16, "A1": 16, "part": 16})
    calls["moka_cross_fwd"] = (
        dict(part=inp((ks, T, RP), f32), Bw=inp((d_out, r)), **{f"A{m}": inp((r, d_in)) for m in range(M)}, h=out((T, RP), f32), hp=out((T, RP), f32),
             hp_tok=out((Tp, 2 * RP)), hp_kmj=out((2, RP, Tp)), BwT=out((RP, d_out)), AT=out((M, d_in, RP))),
        lambda p: lib.moka_cross_fwd(p("part"), ks, byref(rt.struct), s_out, p("Bw"), d_out, _vp([p(f"A{m}") for m in range(M)]), d_in,
                                     p("h"), p("hp"), p("hp_tok"), p("hp_kmj"), p("BwT"), p("AT"), r, spec.w, spec.inv_sqrt_dk, _stream()),
        {k: 16 for k in ("part", "Bw", "A0", "h", "hp", "hp_tok", "hp_kmj", "BwT", "AT")})
    calls["moka_up_fwd"] = (
        dict(hp_tok=inp((Tp, 2 * RP)), Bw=inp((d_out, r)), y=io((T, d_out))),
        lambda p: lib.moka_up_fwd(p("hp_tok"), p("Bw"), rt.tok_mod.data_ptr(), p("y"), T, r, d_out, L.MOKA_BF16, _stream()),
        {"hp_tok": 16, "Bw": 16, "y": 16})
    calls["moka_up_fwd_fused"] = (
        dict(part=inp((ks, T, RP), f32), Bw=inp((d_out, r)), y=io((T, d_out)), h=out((T, RP), f32), hp_kmj=out((2, RP, Tp))),
        lambda p: lib.moka_up_fwd_fused(p("part"), ks, byref(rt.struct), s_out, p("Bw"), p("y"), d_out, p("h"), p("hp_kmj"), r, spec.w,
                                        spec.inv_sqrt_dk, L.MOKA_BF16, _stream()),
        {k: 16 for k in ("part", "Bw", "y", "h", "hp_kmj")})
    calls["moka_weight_shadows"] = (
        dict(Bw=inp((d_out, r)), **{f"A{m}": inp((r, d_in)) for m in range(M)}, BwT=out((RP, d_out)), AT=out((M, d_in, RP))),
        lambda p: lib.moka_weight_shadows(p("Bw"), d_out, _vp([p(f"A{m}") for m in range(M)]), d_in, p("BwT"), p("AT"), r, M, _stream()),
        {"Bw": 16, "A2": 16, "BwT": 16, "AT": 16})
    calls["moka_up_bwd"] = (
        dict(gy=inp((T, d_out)), hp_kmj=inp((2, RP, Tp)), BwT=inp((RP, d_out)), g_part=out((ksb, T, RP), f32), dB=io((d_out, r), f32)),
        lambda p: lib.moka_up_bwd(p("gy"), p("hp_kmj"), p("BwT"), rt.tok_mod.data_ptr(), s_out, p("g_part"), p("dB"), T, r, d_out, M,
                                  L.MOKA_BF16, None, _stream()),
        {"gy": 16, "hp_kmj": 16, "BwT": 16, "g_part": 16, "dB": 4})
    ws_n = int(lib.moka_cross_ws_bytes(c.B, c.S, rt.Lk_max, r))
    calls["moka_cross_bwd"] = (
        dict(g_part=inp((ksb, T, RP), f32), h=inp((T, RP), f32), dh=out((T, RP), f32), dh_tok=out((Tp, 2 * RP)), dh_kmj=out((M, 2, RP, Tp)),
             ws=Buf((max(ws_n, 256),), torch.uint8, "workspace")),
        lambda p: lib.moka_cross_bwd(p("g_part"), ksb, p("h"), byref(rt.struct), spec.s_in, p("dh"), p("dh_tok"), p("dh_kmj"), p("ws"), r,
                                     spec.w, spec.inv_sqrt_dk, _stream()),
        {k: 16 for k in ("g_part", "h", "dh", "dh_tok", "dh_kmj", "ws")})
    calls["moka_down_bwd"] = (
        dict(dh_tok=inp((Tp, 2 * RP)), dh_kmj=inp((M, 2, RP, Tp)), x=inp((T, d_in)), AT=inp((M, d_in, RP)), dx=io((T, d_in)),
             **{f"dA{m}": io((r, d_in), f32) for m in range(M)}),
        lambda p: lib.moka_down_bwd(p("dh_tok"), p("dh_kmj"), p("x"), p("AT"), rt.tok_mod.data_ptr(), _vp([p(f"dA{m}") for m in range(M)]),
                                    p("dx"), T, d_in, r, M, 0.0, 0, L.MOKA_BF16, None, _stream()),
        {"dh_tok": 16, "dh_kmj": 16, "x": 16, "AT": 16, "dx": 16, "dA1": 4})
    return calls


ABI_OPERANDS = {
    "moka_down_fwd": ["x", "A1", "part"],
    "moka_cross_fwd": ["part", "Bw", "A0", "h", "hp", "hp_tok", "hp_kmj", "BwT", "AT"],
    "moka_up_fwd": ["hp_tok", "Bw", "y"],
    "moka_up_fwd_fused": ["part", "Bw", "y", "h", "hp_kmj"],
    "moka_weight_shadows": ["Bw", "A2", "BwT", "AT"],
    "moka_up_bwd": ["gy", "hp_kmj", "BwT", "g_part", "dB"],
    "moka_cross_bwd": ["g_part", "h", "dh", "dh_tok", "dh_kmj", "ws"],
    "moka_down_bwd": ["dh_tok", "dh_kmj", "x", "AT", "dx", "dA1"],
}


@pytest.mark.parametrize("entry,operand", [(e, o) for e, ops in ABI_OPERANDS.items() for o in ops])
def test_c_abi_refuses_a_misaligned_pointer_before_launching_anything(entry, operand):
    """Every device pointer of the adapter entry points, moved off its requirement (16 bytes: by one element and by 8 bytes; the fp32
    accumulators, 4 bytes: by 2 bytes): MOKA_EINVAL, an alignment message naming the argument, and every byte of the arena --
    outputs, accumulators and guard bands -- is what it was before the call."""
    spec, call, need = _abi_calls()[entry]
    assert set(need) == set(ABI_OPERANDS[entry])
    from moka_amd import _lib as L
    lib = L.load()
    b = spec[operand]
    offs = (2,) if need[operand] == 4 else sorted({b.esize, 8})
    for off in offs:
        a = Arena(_dev(), spec, shift=0, seed=1)
        torch.cuda.synchronize()
        rc = call(lambda n: a.ptr(n) + (off if n == operand else 0))
        msg = lib.moka_last_error().decode()
        torch.cuda.synchronize()
        assert rc == EINVAL, f"{entry}({operand} + {off} B): rc={rc} {msg}"
        assert "aligned" in msg and f"{need[operand]}-byte" in msg, msg
        assert torch.equal(a.mem, a.before), f"{entry}({operand} + {off} B): the refused call wrote to its buffers"
    # and the same call on the arena's own (aligned) pointers is accepted
    a = Arena(_dev(), spec, shift=0, seed=1)
    rc = call(a.ptr)
    torch.cuda.synchronize()
    assert rc == 0, f"{entry}: rc={rc} {lib.moka_last_error().decode()}"
    assert not a.guard_damage()


# ==========================================================================================
# 1d. one node for 1..G projections: a group of one, kept shadows on the three-launch path, the refusal
# ==========================================================================================
def _grads_of(ys, x, projs):
    return dict(y=[y.detach() for y in ys], dx=x.grad, dB=[p[2].grad for p in projs], dA=[[a.grad for a in p[3]] for p in projs])


def _assert_same_run(tag, a, b):
    for g, (ya, yb) in enumerate(zip(a["y"], b["y"])):
        assert torch.equal(ya, yb), f"{tag}: y[{g}] differs"
    assert torch.equal(a["dx"], b["dx"]), f"{tag}: dx differs"
    for g, (ga, gb) in enumerate(zip(a["dB"], b["dB"])):
        assert torch.equal(ga, gb), f"{tag}: dB[{g}] differs"
    for g, (la, lb) in enumerate(zip(a["dA"], b["dA"])):
        for m, (ga, gb) in enumerate(zip(la, lb)):
            assert torch.equal(ga, gb), f"{tag}: dA[{g}][{m}] differs"


def _group_of_one_vs_single(name, dt):
    from moka_amd.functional import moka_linear, moka_linear_group
    dev = _dev()
    cd = _cd(name)
    spec0, rt, _ = _srt(name)

    def run(as_group):
        x = _leaf(cd.x, dev, dt)
        p = (cd.W.to(dev, dt), None, _leaf(cd.Bw, dev, dt), [_leaf(a, dev, dt) for a in cd.A])
        spec = _spec(spec0, dropout_p=0.1, seed=0x5eed1 + cd.case.seed)
        y = moka_linear_group(x, [p], rt, [spec])[0] if as_group else moka_linear(x, *p, rt, spec)
        y.backward(cd.gy.to(dev, dt))
        torch.cuda.synchronize()
        return _grads_of([y], x, [p])

    with _Det():
        _assert_same_run(f"{name} {dt} group of one vs single", run(True), run(False))


@pytest.mark.parametrize("fuse", [True, False], ids=["fused", "three_launch"])
@pytest.mark.parametrize("name", CASES)
def test_a_group_of_one_is_the_single_call(name, fuse):
    """moka_linear_group(x, [p], rt, [spec]) and moka_linear(x, *p, rt, spec) on the same inputs, seed and dropout 0.1, deterministic
    weight gradients: y, dx, dB and every dA_m are the same bits, with both forwards."""
    with _Fuse(fuse):
        _group_of_one_vs_single(name, bf)


def test_a_group_of_one_is_the_single_call_fp32_storage():
    """The same with fp32 storage: moka_linear_group sends fp32 calls to the node one projection at a time."""
    _group_of_one_vs_single("avt_r8", f32)


@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("name", ["avt_r16_q", "avt_r64"], ids=["r16", "r64"])          # rank pads 16 and 64 (64 never takes the fused path)
def test_kept_shadows_on_the_three_launch_path(name, G):
    """spec.shadows = (BwT_g, AT_g) of weight_shadows_group for every member, three-launch forward: the same y, dx and (deterministic)
    weight gradients as the call that computes its shadows, and the node writes neither into the shadows it was handed nor around them
    (they sit in guard-banded buffers: every byte of the arena is what it was before the call)."""
    from moka_amd import functional as F
    dev = _dev()
    cds, spec0, rt, _, _ = _group(name, 3)
    cds = cds[:G]

    def run(shadows):
        x = _leaf(cds[0].x, dev)
        projs = [(cd.W.to(dev, bf), None, _leaf(cd.Bw, dev), [_leaf(a, dev) for a in cd.A]) for cd in cds]
        ys = F.moka_linear_group(x, projs, rt, [_spec(spec0, shadows=None if shadows is None else shadows[g]) for g in range(G)])
        torch.autograd.backward(ys, [cd.gy.to(dev, bf) for cd in cds])
        torch.cuda.synchronize()
        return _grads_of(ys, x, projs)

    BwTs, ATs = F.weight_shadows_group([cd.Bw.to(dev, bf) for cd in cds], [[a.to(dev, bf) for a in cd.A] for cd in cds], spec0.r)
    bufs = {}
    for g in range(G):
        bufs[f"BwT{g}"] = Buf(tuple(BwTs[g].shape), bf, "input", data=BwTs[g])
        bufs[f"AT{g}"] = Buf(tuple(ATs[g].shape), bf, "input", data=ATs[g])
    arena = Arena(dev, bufs)
    with _Fuse(False), _Det():
        kept = run([(arena.view(f"BwT{g}"), arena.view(f"AT{g}")) for g in range(G)])
        own = run(None)
    _assert_same_run(f"{name} G={G} kept shadows vs computed", kept, own)
    assert torch.equal(arena.mem, arena.before), f"{name} G={G}: the node wrote into or around the shadows it was handed"


def test_a_group_member_without_a_base_weight_is_refused(monkeypatch):
    """Two members, one with W = None (the adapter term alone is a call of its own): ValueError before any launch."""
    from moka_amd import functional as F
    dev = _dev()
    cds, spec0, rt, _, _ = _group("avt_tiny", 2)
    projs = [(cd.W.to(dev, bf) if g == 0 else None, None, _leaf(cd.Bw, dev), [_leaf(a, dev) for a in cd.A]) for g, cd in enumerate(cds)]
    launches = []
    check = F._lib.check
    monkeypatch.setattr(F._lib, "check", lambda rc, what: (launches.append(what), check(rc, what))[1])
    with pytest.raises(ValueError, match="base weight"):
        F.moka_linear_group(_leaf(cds[0].x, dev), projs, rt, [_spec(spec0) for _ in cds])
    assert launches == [], f"the refused call launched {launches}"
