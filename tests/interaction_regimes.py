"""Regimes of the rank-space cross-modal softmax, a float32 emulation of the kernels' blocking, and the checks the GPU test applies.

CPU-importable (no GPU, no library load).  Used by tests/test_interaction_regimes_host.py (the generator delivers what it claims, the
emulation passes every regime, every mutant of the emulation is rejected) and tests/test_gpu_interaction_regimes.py (the kernels).

Generator.  A regime is a routing (built through MokaRouting.from_avt_masks / from_vt_masks, so the kernels see exactly what the
product path builds) and rank-space rows h whose logits are chosen on purpose: per sample a direction u, key rows a_j s u, query rows
b_i s u, plus a small generic component; s^2 c = the target max |logit|.  h and the upstream gradient g are held on an integer grid
(20-bit integers times one power of two) and split into ks split-K slices on the same grid, so every fp32 sum of the slices, in any
order, is exact: the kernels' h is the generator's h to the bit, and the fp64 oracle sees the same rows.  Rank pad columns are zero;
rows of no modality hold NaN in every slice (unwritten: consumers treat them as zero).

Emulation.  float32, the kernels' blocking: keys in chunks of 64 with a running (max, sum, O) in the forward
(k_cross.hip moka_cross_fwd_kernel, k_expand.hip moka_yx_kernel); in the backward four 16-key tiles per chunk, one per wave, each wave
with its own running (max, sum, sum p dP), merged in wave order, then a second pass for dq and dK (moka_cross_bwd_kernel).  exp is
emulated as exp2(x * log2 e) in fp32, as __expf runs.  ``MUTANTS`` names the subtly wrong variants the checks must reject.

Checks.  Per sample and per row role (query rows: hp - h and dq; key rows: dK; rows that are both: dq + dK), the relative Frobenius
error against the fp64 term:
        err <= 2^-24 * (C * (1 + L) * F * |mag| / |term|  +  C_ROW * |rows| / |term|)
L = max |logit| of the sample (zero keys included), F = sqrt(1 + Lk / 64) (the number of chunks the running statistics cross),
|rows| the norm of the rows the term is added to (hp, dh: the last fp32 rounding is of the sum, not of the term), |mag| >= |term| the
norm of the magnitudes the term is summed from (|w| P |K|; c |dS| |K|; c |dS|^T |Q| + P^T |dO|, |dS| = P (|dP| + |D|)).  |mag| = |term|
unless the term cancels: at a peaked P the softmax-Jacobian terms dq and the key role of dK are differences of nearly equal numbers
(dP_j - D -> 0), and with equal keys dq is exactly 0 (then the error is measured against |mag|).  C and C_ROW are chosen from the
emulation (tests/test_interaction_regimes_host.py: it passes with at least 4x margin, every mutant fails by more than 10x).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field, replace
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from moka_amd.routing import MokaRouting
from oracle import cases as C
from oracle import moka_oracle as O

U = 2.0 ** -24
KC, KT, NWV = 64, 16, 4                 # keys per chunk, keys per wave tile, waves sharing a chunk in the backward
LOG2E = 1.4426950408889634

# bound constants (see the module docstring); the emulation's observed maxima are reported by the host self-test
C_FWD, C_DQ, C_DK, C_ROW = 8.0, 8.0, 8.0, 4.0
PACK_REL = 2.0 ** -16                   # hi + lo bf16 pack of an fp32 value, per element

MUTANTS = (
    "no_max",              # no max subtraction (exp of the raw logits)
    "drop_zero_keys",      # zero key rows left out of the softmax
    "no_rescale_O",        # forward: O not rescaled when the running max rises
    "no_rescale_l",        # forward: l not rescaled when the running max rises
    "merge_wave0_max",     # backward: the wave merge takes wave 0's max
    "merge_empty_wave",    # backward: a wave without keys enters the merge as if it had seen logit 0
    "pdp_first_chunk",     # backward: sum p dP from the first chunk only
    "rsqrt_r",             # 1/sqrt(r) in place of inv_sqrt_dk
    "no_key_role",         # backward: the key-role term of dK dropped
    "drop_overlap_dq",     # backward: dq of a query row that is also a key row dropped
)


def rank_pad(r: int) -> int:
    return 16 if r <= 16 else (32 if r <= 32 else 64)


# --------------------------------------------------------------------------------------------------------------------------------
# regimes
# --------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Samp:
    """One sample: its token layout (oracle/cases.py kinds) and how its logits are placed.

    mode:  'first' / 'last' / 'at' (arg-max key slot = 0 / Lk - 1 / ``at``), 'rise' (a_j increasing: the running max rises in every
           chunk and wave tile), 'equal' (all keys one row: uniform P at any L), 'zeroq' (query rows zero: logits 0),
           'neg' (every valid key's logit in [-L, -L/2]: the zero key rows hold the mass, AVT), 'allneg' (every logit in [-L, -0.9 L]).
    """
    layout: List[Tuple[str, int]]
    L: float = 3.0
    mode: str = "first"
    at: int = 0


@dataclass
class Regime:
    id: str
    variant: str
    r: int
    ks: int
    w: float
    cmul: float                          # inv_sqrt_dk = cmul / sqrt(r)
    S: int
    samples: List[Samp]
    seed: int = 1

    @property
    def inv_sqrt_dk(self) -> float:
        return self.cmul / math.sqrt(self.r)


def _fill(layout, S):
    n = sum(k for _, k in layout)
    assert n <= S, (layout, S)
    return list(layout) + ([("t", S - n)] if n < S else [])


def _vt(nv, Lk, pre=3, over=0, post_img=0):
    """VT layout with nv image tokens and Lk question tokens; ``over`` of the question tokens are image tokens (kind I), spread
    over the question set; post_img image tokens follow the question."""
    lay = [("t", pre), ("v", nv)]
    if Lk:
        if over:
            step = max(Lk // (over + 1), 1)
            q, left = [], Lk
            for _ in range(over):
                q += [("q", min(step, left - 1)), ("I", 1)]
                left -= min(step, left - 1) + 1
            lay += q + [("q", left)] if left > 0 else q
        else:
            lay += [("q", Lk)]
    if post_img:
        lay += [("t", 2), ("v", post_img)]
    return [(k, n) for k, n in lay if n > 0]


def _avt_span(nv, na, span, zero_every=0, pre=2):
    """AVT layout whose question span is ``span`` tokens long; with zero_every, every zero_every-th span token is a zero key row
    (alternately text that is not question and a question token of no modality)."""
    lay = [("t", pre), ("v", nv), ("a", na)]
    if zero_every:
        k, flip = 0, 0
        body = []
        while k < span:
            n = min(zero_every - 1, span - k - 1) if span - k > 1 else 1
            body.append(("q", n))
            k += n
            if k < span - 1:
                body.append(("t" if flip else "Q", 1))
                flip ^= 1
                k += 1
        if body[-1][0] != "q":
            body.append(("q", 1))
        lay += body
    else:
        lay += [("q", span)]
    return [(k, n) for k, n in lay if n > 0]


def regimes() -> List[Regime]:
    R = []
    # short key lists: one chunk, waves without keys (Lk <= 48), the arg-max inside each 16-key tile
    R.append(Regime("avt_r4_short", "avt", 4, 1, 1.0, 1.0, 53, [
        Samp(_avt_span(9, 5, 1), 30, "first"),
        Samp(_avt_span(6, 4, 15), 120, "last"),
        Samp(_avt_span(5, 7, 16), 3, "rise")], seed=11))
    R.append(Regime("vt_r12_tiles", "vt", 12, 3, -1.0, 0.7, 75, [
        Samp(_vt(9, 17), 120, "at", 16),
        Samp(_vt(7, 33), 30, "at", 32),
        Samp(_vt(5, 49), 600, "at", 48),
        Samp(_vt(6, 63), 120, "at", 5)], seed=12))
    # lone key of the last chunk, the running max rising in a later chunk
    R.append(Regime("vt_r16_lone_last", "vt", 16, 7, 4.0, 1.0, 150, [
        Samp(_vt(20, 65), 600, "last"),
        Samp(_vt(10, 129), 120, "last"),
        Samp(_vt(30, 64), 30, "at", 50)], seed=13))
    R.append(Regime("avt_r20_rise", "avt", 20, 3, 0.05, 1.3, 163, [
        Samp(_avt_span(10, 11, 127), 120, "rise"),
        Samp(_avt_span(12, 9, 128), 600, "rise")], seed=14))
    R.append(Regime("vt_r32_long", "vt", 32, 1, 1.0, 0.5, 650, [
        Samp(_vt(40, 200), 120, "at", 150),
        Samp(_vt(30, 600), 600, "rise")], seed=15))
    R.append(Regime("avt_r16_600", "avt", 16, 3, 1.0, 1.0, 700, [
        Samp(_avt_span(30, 20, 600, zero_every=7), 600, "at", 421)], seed=16))
    # zero key rows hold > 99 % of the mass: every valid key's logit <= -40
    R.append(Regime("avt_r48_zero_keys", "avt", 48, 3, 1.0, 1.0, 110, [
        Samp(_avt_span(20, 12, 70, zero_every=4), 120, "neg"),
        Samp(_avt_span(8, 8, 33, zero_every=3), 600, "neg"),
        Samp([("t", 3), ("v", 9), ("q", 4), ("t", 3), ("Q", 2), ("q", 5), ("a", 4)], 120, "neg")], seed=17))
    # every logit far below zero, no zero keys: the running max is the only thing that keeps l finite
    R.append(Regime("vt_r64_allneg", "vt", 64, 7, 1.0, 1.0, 121, [
        Samp(_vt(12, 40), 600, "allneg"),
        Samp(_vt(10, 33), 120, "allneg"),
        Samp(_vt(9, 100), 600, "allneg")], seed=18))
    # near-uniform: equal keys, zero query rows
    R.append(Regime("vt_r16_uniform", "vt", 16, 1, 1.0, 1.0, 93, [
        Samp(_vt(9, 65), 3, "equal"),
        Samp(_vt(11, 16), 0, "zeroq"),
        Samp(_vt(9, 48), 30, "equal")], seed=19))
    # B = 8: samples without keys, without queries, and every regime side by side; 128-token blocks span several samples
    R.append(Regime("vt_r8_mixed_b8", "vt", 8, 3, 1.0, 1.0, 75, [
        Samp([("t", 10), ("q", 9), ("t", 20)]),                       # no image: no keys
        Samp(_vt(12, 0)),                                              # no question
        Samp(_vt(9, 17), 600, "last"),
        Samp(_vt(6, 1), 30, "first"),
        Samp(_vt(7, 65, over=3), 120, "at", 64),
        Samp(_vt(4, 49), 0, "zeroq"),
        Samp(_vt(8, 30), 120, "allneg"),
        Samp([("p", 20), ("t", 3), ("v", 5), ("q", 20)], 3, "rise")], seed=20))
    R.append(Regime("avt_r4_mixed_b8", "avt", 4, 1, -1.0, 1.7, 45, [
        Samp([("t", 3), ("q", 6), ("t", 5)], 30, "first"),            # no query rows
        Samp(_avt_span(8, 4, 20), 600, "at", 17),
        Samp(_avt_span(3, 3, 1), 120, "first"),
        Samp(_avt_span(5, 5, 30, zero_every=5), 120, "neg"),
        Samp([("p", 7)] + _avt_span(6, 0, 10), 3, "rise"),
        Samp(_avt_span(0, 9, 33), 30, "last"),
        Samp(_avt_span(4, 4, 16), 0, "zeroq"),
        Samp(_avt_span(2, 2, 37), 120, "at", 35)], seed=21))
    # query rows that are key rows (VT: image tokens inside the question set), Lk > 64, at every rank pad
    for r, L, seed in ((8, 120, 22), (24, 30, 23), (56, 600, 24)):
        R.append(Regime(f"vt_r{r}_overlap", "vt", r, 3, 1.0, 1.0, 173, [
            Samp(_vt(20, 90, over=5, post_img=8), L, "at", 70),
            Samp(_vt(16, 130, over=9), L, "rise"),
            Samp(_vt(12, 70, over=2), 3, "first")], seed=seed))
    return R


def group_regimes() -> List[Tuple[Regime, List[Regime]]]:
    """(id, three projections in one launch): one routing, each projection in its own logit regime."""
    out = []
    for base in ("vt_r16_lone_last", "avt_r20_rise", "vt_r56_overlap"):
        reg = next(x for x in regimes() if x.id == base)
        projs = []
        for gi, (L, mode) in enumerate(((3.0, "first"), (120.0, "rise"), (600.0, "last"))):
            projs.append(replace(reg, id=f"{base}_g{gi}", seed=reg.seed * 10 + gi,
                                 samples=[replace(s, L=L if s.L else 0.0, mode=mode if s.mode not in ("zeroq", "equal", "neg", "allneg") else s.mode)
                                          for s in reg.samples]))
        out.append((base, projs))
    return out


# --------------------------------------------------------------------------------------------------------------------------------
# data
# --------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Data:
    reg: Regime
    masks: list                          # reference-format masks (CPU)
    ort: O.Routing                       # the oracle's routing
    rt: MokaRouting                      # the kernels' routing (CPU tensors)
    B: int
    S: int
    T: int
    r: int
    RP: int
    h: torch.Tensor                      # [T, RP] fp32, exact
    part: torch.Tensor                   # [ks, T, RP] fp32 slices (NaN rows of no modality)
    g: torch.Tensor                      # [T, RP] fp32, exact
    g_part: torch.Tensor                 # [ks, T, RP]
    is_query: torch.Tensor               # [T] bool
    is_key: torch.Tensor                 # [T] bool (a live key row)
    has_mod: torch.Tensor                # [T] bool
    ref: Dict[str, torch.Tensor] = field(default_factory=dict)    # fp64: hp, dq, dk, dh  ([T, r])
    L: List[float] = field(default_factory=list)                   # per sample: max |logit| (0 without queries / keys)
    mag: Dict[str, torch.Tensor] = field(default_factory=dict)     # fp64 magnitudes of the terms (see make)
    logits: List[Optional[torch.Tensor]] = field(default_factory=list)


def _masks(variant, tok_mod, question):
    if variant == "avt":
        return [(tok_mod == m).to(torch.int32).unsqueeze(-1) for m in range(3)] + [question.to(torch.int32).unsqueeze(-1)]
    return [tok_mod == C.TEXT, tok_mod == C.VIS, question]


def _grid(x: torch.Tensor, ks: int, gen: torch.Generator, valid: torch.Tensor):
    """x [T, RP] fp64 -> (exact fp32 rows, [ks, T, RP] slices): 20-bit integers times one power of two."""
    mx = float(x.abs().max())
    e = (math.floor(math.log2(mx)) - 19) if mx > 0 else 0
    q = 2.0 ** e
    xi = torch.round(x / q)
    sl = []
    rest = xi.clone()
    for _ in range(ks - 1):
        s = torch.randint(-2 ** 20, 2 ** 20 + 1, x.shape, generator=gen).double() * (xi != 0)
        sl.append(s)
        rest = rest - s
    sl.append(rest)
    part = (torch.stack(sl) * q).float()
    part[:, ~valid] = float("nan")
    exact = (xi * q).float()
    exact[~valid] = 0.0
    return exact, part


def make(reg: Regime) -> Data:
    gen = torch.Generator().manual_seed(reg.seed)
    B, S, r = len(reg.samples), reg.S, reg.r
    RP, T = rank_pad(r), B * S
    tm, qq = [], []
    for s in reg.samples:
        t, q = C.build_layout(_fill(s.layout, S), S)
        tm.append(t)
        qq.append(q)
    tok_mod, question = torch.stack(tm), torch.stack(qq)
    masks = _masks(reg.variant, tok_mod, question)
    if reg.variant == "avt":
        ort = O.routing_from_avt_masks(masks)
        rt = MokaRouting.from_avt_masks(masks)
    else:
        ort = O.routing_from_vt_masks(*masks)
        rt = MokaRouting.from_vt_masks(*masks)
    c = reg.inv_sqrt_dk
    h = torch.zeros(B, S, RP, dtype=torch.float64)
    h[..., :r] = torch.randn(B, S, r, generator=gen, dtype=torch.float64)
    for b, smp in enumerate(reg.samples):
        kp, kv = ort.kpos[b], ort.kvalid[b]
        qrows = torch.where(ort.is_query[b])[0]
        Lk = kp.numel()
        if Lk == 0 or qrows.numel() == 0:
            continue
        u = torch.randn(r, generator=gen, dtype=torch.float64)
        u /= u.norm()
        sc = math.sqrt(smp.L / c) if smp.L > 0 else 1.0
        noise = lambda n, d=0.01: d * sc * torch.randn(n, r, generator=gen, dtype=torch.float64) / math.sqrt(r)   # noqa: E731
        rnd = lambda n, lo, hi: lo + (hi - lo) * torch.rand(n, generator=gen, dtype=torch.float64)              # noqa: E731
        beta = rnd(qrows.numel(), 0.8, 1.0)
        beta[0] = 1.0
        if smp.mode == "zeroq":
            h[b, qrows, :r] = 0.0
        else:
            h[b, qrows, :r] = sc * beta[:, None] * u[None, :] + noise(qrows.numel())
        if smp.mode == "zeroq":
            a = None
        elif smp.mode == "equal":
            a = torch.ones(Lk, dtype=torch.float64)
        elif smp.mode == "neg":
            a = rnd(Lk, -1.0, -0.5)
        elif smp.mode == "allneg":
            a = rnd(Lk, -1.0, -0.9)
        elif smp.mode == "rise":
            a = torch.linspace(-1.0, 1.0, Lk + 1, dtype=torch.float64)[1:]
        else:
            a = rnd(Lk, -1.0, 0.8)
            j = {"first": 0, "last": Lk - 1, "at": smp.at}[smp.mode]
            assert bool(kv[j]), (reg.id, b, j)
            a[j] = 1.0
        if smp.mode in ("neg", "allneg"):
            a[int(torch.where(kv)[0][-1])] = -1.0        # (the largest |logit| is the target)
        if a is not None:
            K = sc * a[:, None] * u[None, :]
            K = K + (0.0 if smp.mode == "equal" else noise(Lk))
            if smp.mode == "equal":
                K = K + noise(1)
            h[b, kp[kv], :r] = K[kv]               # (query rows that are key rows: the key pattern wins)
    valid = (tok_mod >= 0).reshape(T)
    h2, part = _grid(h.reshape(T, RP), reg.ks, gen, valid)
    g = torch.zeros(T, RP, dtype=torch.float64)
    g[:, :r] = torch.randn(T, r, generator=gen, dtype=torch.float64)
    g2, g_part = _grid(g, reg.ks, gen, valid)
    is_key = torch.zeros(T, dtype=torch.bool)
    kt = rt.ktok
    for b in range(B):
        k = kt[b, :int(rt.klen[b])]
        is_key[k[k >= 0].long()] = True
    d = Data(reg, masks, ort, rt, B, S, T, r, RP, h2, part, g2, g_part, ort.is_query.reshape(T).clone(), is_key, valid)
    # fp64 oracle
    h64 = h2[:, :r].double().reshape(B, S, r)
    ia = O.interaction_forward(h64, ort, reg.w, c)
    dh, dq, dk = O.interaction_backward(g2[:, :r].double().reshape(B, S, r), ia)
    d.ref = {"hp": ia.hp.reshape(T, r), "dh": dh.reshape(T, r), "dq": dq.reshape(T, r), "dk": dk.reshape(T, r)}
    # magnitudes the terms are computed from (|w| P |K|, c |dS| |K|, c |dS|^T |Q| + P^T |dO| with |dS| = P (|dP| + |D|)): the
    # scale of a term's rounding error where the term itself cancels (peaked P: dP_j - D -> 0; equal keys: dq = 0)
    mag = {k: torch.zeros(B, S, r, dtype=torch.float64) for k in ("hp", "dq", "dk")}
    g64 = g2[:, :r].double().reshape(B, S, r)
    for b in range(B):
        if ia.P[b] is None:
            d.L.append(0.0)
            d.logits.append(None)
            continue
        P = ia.P[b]
        kp, kv = ort.kpos[b], ort.kvalid[b].double()[:, None]
        qrows = torch.where(ort.is_query[b])[0]
        K = h64[b, kp] * kv
        Q, dO = h64[b, qrows], reg.w * g64[b, qrows]
        lg = (Q @ K.t()) * c
        d.logits.append(lg)
        d.L.append(float(lg.abs().max()))
        dP = dO @ K.t()
        dSm = P * (dP.abs() + (P * dP).sum(-1, keepdim=True).abs())
        mag["hp"][b, qrows] = abs(reg.w) * (P @ K.abs())
        mag["dq"][b, qrows] = c * (dSm @ K.abs())
        mag["dk"][b].index_add_(0, kp, (c * (dSm.t() @ Q.abs()) + P.t() @ dO.abs()) * kv)
    d.mag = {k: v.reshape(T, r) for k, v in mag.items()}
    return d


# --------------------------------------------------------------------------------------------------------------------------------
# float32 emulation of the kernels' blocking
# --------------------------------------------------------------------------------------------------------------------------------
def _exp(x: torch.Tensor) -> torch.Tensor:
    return torch.exp2(x * torch.tensor(LOG2E, dtype=torch.float32))


def _sample_rows(d: Data, b: int):
    Lk = int(d.rt.klen[b])
    rows = torch.arange(b * d.S, (b + 1) * d.S)
    tm = d.rt.tok_mod[rows].long()
    q = rows[(tm == 1) | (tm == 2)]
    kt = d.rt.ktok[b, :Lk].long()
    return Lk, q, kt


def _keys(h: torch.Tensor, kt: torch.Tensor) -> torch.Tensor:
    K = h[kt.clamp(min=0)].clone()
    K[kt < 0] = 0.0
    return K


def _c32(d: Data, mut) -> torch.Tensor:
    c = 1.0 / math.sqrt(d.r) if "rsqrt_r" in mut else d.reg.inv_sqrt_dk
    return torch.tensor(c, dtype=torch.float32)


def emulate_forward(d: Data, mut: Sequence[str] = ()) -> torch.Tensor:
    """hp [T, RP] fp32 as the forward kernels compute it (key chunks of 64, running max / sum / O)."""
    h = d.h
    hp = h.clone()
    c = _c32(d, mut)
    w = torch.tensor(d.reg.w, dtype=torch.float32)
    for b in range(d.B):
        Lk, q, kt = _sample_rows(d, b)
        if Lk == 0 or q.numel() == 0:
            continue
        Q, K = h[q], _keys(h, kt)
        m = torch.full((q.numel(),), -math.inf)
        l = torch.zeros(q.numel())
        Ov = torch.zeros(q.numel(), d.RP)
        for c0 in range(0, Lk, KC):
            Kc = K[c0:c0 + KC]
            s = (Q @ Kc.t()) * c
            if "drop_zero_keys" in mut:
                s[:, kt[c0:c0 + KC] < 0] = -math.inf
            m_new = torch.maximum(m, s.max(1).values)
            if "no_max" in mut:
                m_new = torch.zeros_like(m_new)
            alpha = _exp(m - m_new)
            p = _exp(s - m_new[:, None])
            l = (l if "no_rescale_l" in mut else l * alpha) + p.sum(1)
            Ov = (Ov if "no_rescale_O" in mut else Ov * alpha[:, None]) + p @ Kc
            m = m_new
        hp[q] = h[q] + (w / l)[:, None] * Ov
    return hp


def emulate_backward(d: Data, h: Optional[torch.Tensor] = None, mut: Sequence[str] = ()) -> torch.Tensor:
    """dh [T, RP] fp32 as moka_cross_bwd computes it: pass 1 per-wave running (max, sum, sum p dP) over 16-key tiles, merged in wave
    order; pass 2 dq and dK; a key row gets g + sum of its dK (+ its dq when it is also a query row)."""
    h = d.h if h is None else h
    g = d.g
    dh = g.clone()
    c = _c32(d, mut)
    w = torch.tensor(d.reg.w, dtype=torch.float32)
    for b in range(d.B):
        Lk, q, kt = _sample_rows(d, b)
        if Lk == 0 or q.numel() == 0:
            continue
        nq = q.numel()
        Q, K, dO = h[q], _keys(h, kt), w * g[q]
        zero_key = kt < 0
        mw = torch.full((NWV, nq), -math.inf)
        lw = torch.zeros(NWV, nq)
        nw = torch.zeros(NWV, nq)
        for c0 in range(0, Lk, KC):
            for wv in range(NWV):
                j0, j1 = c0 + KT * wv, min(c0 + KT * (wv + 1), Lk)
                if j0 >= j1:
                    continue
                Kt = K[j0:j1]
                s = (Q @ Kt.t()) * c
                if "drop_zero_keys" in mut:
                    s[:, zero_key[j0:j1]] = -math.inf
                dp = dO @ Kt.t()
                m_new = torch.maximum(mw[wv], s.max(1).values)
                if "no_max" in mut:
                    m_new = torch.zeros_like(m_new)
                ok = m_new > -math.inf
                alpha = torch.where(ok, _exp(mw[wv] - m_new), torch.ones_like(m_new))
                p = torch.where(ok[:, None], _exp(s - m_new[:, None]), torch.zeros_like(s))
                lw[wv] = lw[wv] * alpha + p.sum(1)
                if c0 == 0 or "pdp_first_chunk" not in mut:
                    nw[wv] = nw[wv] * alpha + (p * dp).sum(1)
                mw[wv] = torch.where(ok, m_new, mw[wv])
        if "merge_empty_wave" in mut:
            mw = torch.where(torch.isinf(mw) & (mw < 0), torch.zeros_like(mw), mw)
        m_run = mw[0].clone() if "merge_wave0_max" in mut else mw.max(0).values
        if "no_max" in mut:
            m_run = torch.zeros_like(m_run)
        l = torch.zeros(nq)
        n = torch.zeros(nq)
        for wv in range(NWV):
            sc = torch.where(mw[wv] > -math.inf, _exp(mw[wv] - m_run), torch.zeros_like(m_run))
            l = lw[wv] * sc + l
            n = nw[wv] * sc + n
        inv_l = 1.0 / l
        D = n * inv_l
        dq = torch.zeros(nq, d.RP)
        dK = torch.zeros(Lk, d.RP)
        for c0 in range(0, Lk, KC):
            Kc = K[c0:c0 + KC]
            s = (Q @ Kc.t()) * c
            if "drop_zero_keys" in mut:
                s[:, zero_key[c0:c0 + KC]] = -math.inf
            dp = dO @ Kc.t()
            P = _exp(s - m_run[:, None]) * inv_l[:, None]
            dS = P * (dp - D[:, None]) * c
            dq += dS @ Kc
            dK[c0:c0 + KC] = (P.t() @ dO) if "no_key_role" in mut else (dS.t() @ Q + P.t() @ dO)
        dh[q] = g[q] + dq
        live = kt >= 0
        for j in torch.where(live)[0].tolist():
            t = int(kt[j])
            extra = dh[t] - g[t] if (bool(d.is_query[t]) and "drop_overlap_dq" not in mut) else 0.0
            dh[t] = (dK[j] + extra) + g[t]
    return dh


# --------------------------------------------------------------------------------------------------------------------------------
# checks
# --------------------------------------------------------------------------------------------------------------------------------
def _size(Lk: int) -> float:
    return math.sqrt(1.0 + Lk / KC)


def _err_bound(Cr: float, L: float, Lk: int, got: torch.Tensor, term: torch.Tensor, mag: torch.Tensor, rows: torch.Tensor):
    """(err, bound) relative to |term|; |mag| >= |term| stands in where the term cancels (|term| < |mag|: the bound's first part
    scales with |mag| / |term|; a term that is exactly 0 is measured against |mag| instead)."""
    nt, nm = float(term.norm()), float(mag.norm())
    den = nt if nt > 0 else nm
    if den == 0:
        return (0.0 if float(got.norm()) == 0 else math.inf), U
    e = float((got - term).norm()) / den if bool(torch.isfinite(got).all()) else math.inf
    return e, U * (Cr * (1.0 + L) * _size(Lk) * nm + C_ROW * float(rows.norm())) / den


def forward_errors(d: Data, hp: torch.Tensor) -> List[dict]:
    """Per sample with queries and keys: the error of hp - h on its query rows against the fp64 term, with its bound."""
    hp = hp.double().cpu()
    out = []
    for b in range(d.B):
        Lk, q, _ = _sample_rows(d, b)
        if Lk == 0 or q.numel() == 0:
            continue
        r = d.r
        term = d.ref["hp"][q] - d.h[q, :r].double()
        got = hp[q, :r] - d.h[q, :r].double()
        e, bd = _err_bound(C_FWD, d.L[b], Lk, got, term, d.mag["hp"][q], d.ref["hp"][q])
        out.append(dict(sample=b, role="hp-h", Lk=Lk, L=d.L[b], err=e, bound=bd))
    return out


def backward_errors(d: Data, dh: torch.Tensor) -> List[dict]:
    """Per sample and row role: query rows (dq), key rows (dK), rows that are both (dq + dK), on dh - g against the fp64 terms."""
    dh = dh.double().cpu()
    r = d.r
    out = []
    for b in range(d.B):
        Lk, q, _ = _sample_rows(d, b)
        if Lk == 0 or q.numel() == 0:
            continue
        rows = torch.arange(b * d.S, (b + 1) * d.S)
        isq, isk = d.is_query[rows], d.is_key[rows]
        for role, sel, Cr in (("dq", isq & ~isk, C_DQ), ("dK", isk & ~isq, C_DK), ("dq+dK", isq & isk, max(C_DQ, C_DK))):
            t = rows[sel]
            if t.numel() == 0:
                continue
            term = d.ref["dq"][t] + d.ref["dk"][t]
            got = dh[t, :r] - d.g[t, :r].double()
            e, bd = _err_bound(Cr, d.L[b], Lk, got, term, d.mag["dq"][t] + d.mag["dk"][t], d.ref["dh"][t])
            out.append(dict(sample=b, role=role, Lk=Lk, L=d.L[b], err=e, bound=bd))
    return out


def worst(rows: List[dict]) -> float:
    """max err / bound (inf for a non-finite result)."""
    return max((x["err"] / x["bound"] if math.isfinite(x["err"]) else math.inf) for x in rows) if rows else 0.0


def fmt(rows: List[dict]) -> str:
    return "; ".join(f"b{x['sample']} {x['role']} Lk={x['Lk']} L={x['L']:.3g}: {x['err']:.3g} / {x['bound']:.3g}" for x in rows)


def check_forward_exact(d: Data, hp: torch.Tensor) -> None:
    """Rows that are no query rows of a sample with keys keep h to the bit; pad columns are zero; nothing is non-finite."""
    hp = hp.float().cpu()
    assert bool(torch.isfinite(hp).all()), "non-finite hp"
    upd = torch.zeros(d.T, dtype=torch.bool)
    for b in range(d.B):
        Lk, q, _ = _sample_rows(d, b)
        if Lk:
            upd[q] = True
    assert torch.equal(hp[~upd], d.h[~upd]), "hp != h on rows that are not updated"
    if d.RP > d.r:
        assert float(hp[:, d.r:].abs().max()) == 0.0, "hp pad columns"


def check_backward_exact(d: Data, dh: torch.Tensor) -> None:
    """Rows (of a modality) that are neither query nor key rows: dh = g to the bit (g is exact in every summation order)."""
    dh = dh.float().cpu()
    assert bool(torch.isfinite(dh).all()), "non-finite dh"
    plain = d.has_mod & ~d.is_key
    for b in range(d.B):
        Lk, q, _ = _sample_rows(d, b)
        if Lk:
            plain[q] = False
    assert torch.equal(dh[plain], d.g[plain]), "dh != g on rows that are neither query nor key rows"
    if d.RP > d.r:
        assert float(dh[d.has_mod][:, d.r:].abs().max()) == 0.0, "dh pad columns"


def pack_error(pack_sum: torch.Tensor, want: torch.Tensor) -> float:
    """max over elements of |hi + lo - want| / |want| (elements where want == 0 must be exactly 0)."""
    a, b = pack_sum.double().cpu(), want.double().cpu()
    if not bool(torch.isfinite(a).all()):
        return math.inf
    nz = b != 0
    if bool((a[~nz] != 0).any()):
        return math.inf
    return float(((a[nz] - b[nz]).abs() / b[nz].abs()).max()) if bool(nz.any()) else 0.0
