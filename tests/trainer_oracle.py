"""The attach() trainer step against the fp64 oracle (a helper module like ``tests/schedule_oracle.py``, not a conftest).

The path a user trains with -- ``moka_amd.parallel.attach()`` -> ``AdapterDataParallel`` -> ``dp.step()`` / ``GraphedTrainStep`` -- is
compared by the other trainer files with itself.  This harness runs K real optimizer steps of a small model under ``attach()``, records
every adapted call, and says what each step must have computed, whichever way it is implemented:

* RECORD.  ``functional.moka_linear`` / ``moka_linear_group`` are wrapped where the layers look them up (``moka_amd.decoder``,
  ``moka_amd.peft_hyper.lora``, ``moka_amd.modified_peft.layer``).  The wrapper clones x and every y, hooks their gradients and notes
  which parameters and which ``AdapterSpec`` were handed in; it changes nothing the call computes.
* COMPARE (``compare_step``, no GPU needed).  Per call: y and dx against ``_oracle`` of ``tests/test_gpu_autograd_conditions.py`` on the
  recorded x / gy and the working copies as they stood in front of the step.  Per parameter view: the gradient the step consumed, recovered
  from the first moments (``recover_grad``), against coefficient x 1/world x the sum over micro-batches and calls of the oracle's dA_m /
  dB (hooked parameters: what a tensor hook on the parameter saw); the oracle's own clip coefficient; the master against fp64 AdamW with
  the HF no-decay rule restated here (``hf_no_decay``); padding, working copy, weight shadows, counters.

Bounds are the project's: TOL_E2E (y / dx with a base weight), TOL_F32 (kernel-fed gradients), TOL_CAST (hooked bf16 gradients),
TOL_F32_STORAGE, TOL_ADAMW.  The one new figure is TOL_NORM = 1e-5 on the norm ``dp.step`` returns (the fp32 norm of a few 10^5
elements: the accuracy class of TOL_F32_STORAGE); measured on an MI355X: 3.5e-8 (clip active) and 1.1e-7 (inactive).  No oracle value had
to be rounded the way a storage format forces: the hooked bf16 gradients are compared with what a tensor hook on the parameter saw, which
is the bf16 value autograd produced per micro-batch already (measured 1.1e-7 against TOL_CAST = 2e-3).  Every parameter of the model under
test is a multiple of 8 elements long, so the padding rows appear in the CPU emulation only (``ToyTrainer`` pads four of its views).

Scales.  ``lora_B`` and the base weights are drawn with ``STD_W`` and ``std_B(rank)``, chosen from the oracle alone:
``reference_loss`` below is the whole model in fp64 on the CPU (adapters through ``O.adapter_forward``), and with these values it gives
|adapter term| / |base term| between 0.70 and 1.67 for every call of every configuration at the initial weights
(``tests/test_trainer_oracle_host.py`` asserts 0.5 .. 2; the GPU rows assert TERM_LO .. TERM_HI = 0.25 .. 4 per recorded call).  The same
reference gives the gradient norm the clip thresholds are taken from (``CLIP_ACTIVE`` / ``CLIP_INACTIVE``).

Seeded faults.  ``ToyTrainer`` is a plain fp64 / fp32 CPU emulation of a correct step on a 2-projection layout; each ``fault`` makes it
wrong in one way a trainer can be wrong, and ``tests/test_trainer_oracle_host.py`` shows that ``compare_step`` reports the named check
and no unrelated one.  One fault of the list cannot be observed by ANY check of values: decay applied to the padding multiplies exact zeros
(p = g = m = v = 0 gives p = 0 for every weight decay).  What is seeded instead is the fault next to it that does change values: the
decay ranges cut at the UNPADDED offsets (``decay_ignores_padding``), which moves every range by the padding in front of it.
"""
from __future__ import annotations

import contextlib
import importlib
import math
import os
import sys
from typing import Dict, List, NamedTuple, Optional, Sequence

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import moka_oracle as O  # noqa: E402
from tests.schedule_oracle import (M_OVER_G, TERM_HI, TERM_LO, TOL_ADAMW, Row, adamw_fp64, failed, failures, recover_grad, rel,  # noqa: E402,F401
                                   summary, worst)
from tests.test_gpu_autograd_conditions import TOL_CAST, _oracle  # noqa: E402
from tests.test_gpu_parity import TOL_E2E, TOL_F32, TOL_F32_STORAGE, _check_routing  # noqa: E402

TOL_NORM = 1e-5                 # dp.step's returned norm against the fp64 norm of the oracle's mean gradient, relative
NO_CANCEL = 2.0                 # precondition of a relative gradient bound: max_i |g_i| <= 2 |sum_i g_i| over the micro-batches
STD_W = 0.05                    # base weights (what tests/test_gpu_trainer.py's TinyLM draws them with)
ALPHA = 16
B_, S_, FEAT, OUT = 3, 96, 40, 8
CLIP_ACTIVE, CLIP_INACTIVE = 0.01, 100.0        # max_grad_norm; reference_loss gives a gradient norm of 1.3 .. 4.1 per micro-batch at the initial weights


def std_B(rank: int, alpha: float = ALPHA, d_ins: Sequence[int] = (128, 352)) -> float:
    """std of lora_B that makes |adapter term| ~ |base term|: with x of unit rms, A_m kaiming-uniform (std 1 / sqrt(3 d_in)) the rank-space
    rows have std s / sqrt(3) (s = alpha / r) and the term s sqrt(r / 3) std_B; the base has sqrt(d_in) STD_W.  Geometric mean over the
    two input widths of the block."""
    s = float(alpha) / rank
    return STD_W * math.sqrt(3.0) * math.sqrt(math.sqrt(d_ins[0] * d_ins[1])) / (s * math.sqrt(rank))


# ======================================================================================================================================
# layout: where every trainable parameter lives in the flat buffers, and which ones decay -- restated, not read from attach()
# ======================================================================================================================================
class View(NamedTuple):
    name: str
    offset: int
    size: int
    shape: tuple
    kernel: bool                # the weight-gradient kernels write its gradient (a sink); False: an autograd gradient folded in by a hook
    decay: bool
    f32: bool                   # fp32 storage: the parameter is a view of the master, not of the bf16 working copy

    @property
    def end(self) -> int:
        return self.offset + self.size

    @property
    def padded_end(self) -> int:
        return self.offset + (self.size + 7) // 8 * 8


def _is_norm(mod: nn.Module) -> bool:
    return isinstance(mod, (nn.LayerNorm, getattr(nn, "RMSNorm", nn.LayerNorm))) or "norm" in type(mod).__name__.lower()


def hf_no_decay(model: nn.Module) -> set:
    """Names of the parameters HF Trainer's default optimizer trains without weight decay: every parameter of a normalisation layer and
    every parameter whose name contains "bias" (transformers.Trainer.get_decay_parameter_names, from module types and names)."""
    out = set()
    for mod_name, mod in model.named_modules():
        for pn, _ in mod.named_parameters(recurse=False):
            full = (mod_name + "." if mod_name else "") + pn
            if "bias" in full.lower() or _is_norm(mod):
                out.add(full)
    return out


def kernel_fed_names(model: nn.Module) -> set:
    """The adapter matrices of the adapted projections: lora_A{m} / lora_B0 (AVT mirror), lora_A.text / lora_A.image / lora_B.text (VT)."""
    out = set()
    for mod_name, mod in model.named_modules():
        pre = mod_name + "." if mod_name else ""
        if hasattr(mod, "lora_B0"):
            out.add(pre + "lora_B0.weight")
            out.update(pre + "lora_A%d.weight" % i for i in range(mod.lora_num))
        elif isinstance(getattr(mod, "lora_A", None), (dict, nn.ModuleDict)) and "text" in mod.lora_A:
            out.update([pre + "lora_B.text.weight", pre + "lora_A.text.weight", pre + "lora_A.image.weight"])
    return out


def expected_layout(model: nn.Module, layers_prefix: str = "model.layers.") -> List[View]:
    """Module order inside a group; the groups are: everything the kernels do not feed (first), then one per decoder layer; every
    parameter starts at a multiple of 8 elements."""
    fed, nd = kernel_fed_names(model), hf_no_decay(model)
    items = []
    for k, (n, p) in enumerate((n, p) for n, p in model.named_parameters() if p.requires_grad):
        layer = int(n[len(layers_prefix):].split(".")[0]) if (n in fed and n.startswith(layers_prefix)) else -1
        items.append((layer, k, n, p))
    views, off = [], 0
    for layer, _, n, p in sorted(items, key=lambda it: (it[0], it[1])):
        views.append(View(n, off, p.numel(), tuple(p.shape), n in fed, n not in nd, p.dtype == torch.float32))
        off += (p.numel() + 7) // 8 * 8
    return views


# ======================================================================================================================================
# records (CPU tensors) and the comparison
# ======================================================================================================================================
class Member:
    """One projection of a recorded call."""

    def __init__(self, name_B, names_A, W, bias, spec, y=None, gy=None, keep=None, inv_keep=1.0):
        self.name_B, self.names_A, self.W, self.bias, self.spec = name_B, list(names_A), W, bias, spec
        self.y, self.gy, self.keep, self.inv_keep = y, gy, keep, float(inv_keep)


class SpecRec(NamedTuple):
    r: int
    s_in: float
    s_out: tuple
    w: float
    inv_sqrt_dk: float
    dropout_p: float
    seed: int


class Call:
    def __init__(self, micro: int, x, members: List[Member], gx=None, routing=None):
        self.micro, self.x, self.members, self.gx, self.routing = micro, x, members, gx, routing

    @property
    def key(self):
        return tuple(m.name_B for m in self.members)

    @property
    def is_reforward(self) -> bool:
        """A layer's forward run again inside the backward by an activation checkpoint: nothing backpropagates through its outputs."""
        return all(m.gy is None for m in self.members)


class StepCfg(NamedTuple):
    lr: float
    betas: tuple = (0.9, 0.999)
    eps: float = 1e-8
    weight_decay: float = 0.0
    max_grad_norm: Optional[float] = None       # None: the step does not clip
    world: int = 1
    clip_expect: Optional[str] = None           # "active" / "inactive": asserted from the oracle's norm
    f32: bool = False


class _Shape(NamedTuple):
    B: int
    S: int
    r: int


class _CD(NamedTuple):
    case: _Shape


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16)


def compare_step(views: Sequence[View], cfg: StepCfg, k: int, calls: Sequence[Call], hooked: Dict[str, List[torch.Tensor]],
                 before: dict, after: dict, returned_norm: Optional[float]) -> List[Row]:
    """Rows of optimizer step k (1-based).  before / after: dict(master, m, v, work[, grad, t, shadows, grads_set]) of CPU tensors;
    hooked[name] = the gradient a tensor hook on the parameter saw, per micro-batch; returned_norm: what dp.step returned (None: nothing)."""
    R: List[Row] = []
    by = {v.name: v for v in views}
    tol_out = TOL_F32_STORAGE if cfg.f32 else TOL_E2E
    P = {v.name: (before["master"] if v.f32 else before["work"])[v.offset:v.end].double().view(v.shape) for v in views}
    micros = sorted({c.micro for c in calls} | {i for gs in hooked.values() for i in range(len(gs))})
    G = {v.name: {i: torch.zeros(v.shape, dtype=torch.float64) for i in micros} for v in views}

    # ---- per recorded call: y and dx against the fp64 oracle on the recorded x / gy and the working copies in front of the step
    live = [c for c in calls if not c.is_reforward]
    for ci, c in enumerate(live):
        Bc, Sc = c.x.shape[0], c.x.shape[1]
        dx = None
        for mb in c.members:
            sp = mb.spec
            where = "micro%d.%s" % (c.micro, mb.name_B.rsplit(".lora_B", 1)[0])
            R.append(Row(k, "pre.d_k", where, abs(sp.inv_sqrt_dk * math.sqrt(sp.r) - 1.0), 1e-12))
            if mb.gy is None:
                R.append(Row(k, "record", where + ": an output without a gradient", 1.0, 0.0))
                continue
            o = _oracle(_CD(_Shape(Bc, Sc, sp.r)), sp, c.routing, x=c.x, gy=mb.gy.reshape(Bc, Sc, -1), W=mb.W, bias=mb.bias, keep=mb.keep,
                        inv_keep=mb.inv_keep, A=[P[n] for n in mb.names_A], Bw=P[mb.name_B])
            base = c.x.double() @ mb.W.double().t() + (0.0 if mb.bias is None else mb.bias.double())
            t_, b_ = (o.y - base).norm().item(), base.norm().item()
            R.append(Row(k, "pre.term_over_base", where, t_ / b_ if b_ > 0 else float("inf"), TERM_HI))
            R.append(Row(k, "pre.base_over_term", where, b_ / t_ if t_ > 0 else float("inf"), 1.0 / TERM_LO))
            R.append(Row(k, "y", where, rel(mb.y.reshape(Bc, Sc, -1), o.y), tol_out))
            dx = o.dx if dx is None else dx + o.dx
            for n, g in zip(mb.names_A, o.dA):
                G[n][c.micro] += g
            G[mb.name_B][c.micro] += o.dB
        if dx is not None:
            where = "micro%d.%s" % (c.micro, "+".join(m.name_B.rsplit(".lora_B", 1)[0].rsplit(".", 1)[-1] for m in c.members) + "@" +
                                    c.members[0].name_B.rsplit(".lora_B", 1)[0].rsplit(".", 1)[0])
            if c.gx is None:
                R.append(Row(k, "record", where + ": no gradient reached x", 1.0, 0.0))
            else:
                R.append(Row(k, "dx", where, rel(c.gx.reshape(Bc, Sc, -1), dx), tol_out))

    # ---- an activation checkpoint records every call twice; the re-forward's x is the first record's, bit for bit
    refwd = [c for c in calls if c.is_reforward]
    for c in refwd:
        first = [d for d in live if d.key == c.key and d.micro == c.micro]
        bad = 1.0 if len(first) != 1 else float(not torch.equal(first[0].x, c.x)) + float(
            any(a.spec.seed != b.spec.seed for a, b in zip(first[0].members, c.members)))
        R.append(Row(k, "ckpt.x_equal", "micro%d.%s" % (c.micro, c.key[0]), bad, 0.0))

    # ---- the mean gradient, its norm and the clip coefficient: the oracle's own
    for n, gs in hooked.items():
        for i, g in enumerate(gs):
            G[n][i] += g.double().reshape(by[n].shape)
    mean = {n: sum(G[n].values()) / cfg.world if G[n] else torch.zeros(by[n].shape, dtype=torch.float64) for n in G}
    norm = math.sqrt(sum(float(g.pow(2).sum()) for g in mean.values()))
    coef = 1.0
    if cfg.max_grad_norm is not None and cfg.max_grad_norm > 0:
        coef = min(1.0, cfg.max_grad_norm / (norm + 1e-6))
        if returned_norm is None:
            R.append(Row(k, "clip.norm", "nothing returned", float("inf"), TOL_NORM))
        else:
            R.append(Row(k, "clip.norm", "returned %.9g oracle %.9g" % (returned_norm, norm), abs(returned_norm - norm) / norm, TOL_NORM))
        if cfg.clip_expect == "active":
            R.append(Row(k, "pre.clip_active", "coefficient", coef, 0.7))
        elif cfg.clip_expect == "inactive":
            R.append(Row(k, "pre.clip_inactive", "norm / max_norm", norm / cfg.max_grad_norm, 0.5))

    # ---- the gradient the step consumed, per parameter view (what it did not consume is still in the buffer and fails grad_left_zero)
    gbuf = after["grad"].double() if after.get("grad") is not None else torch.zeros_like(after["m"], dtype=torch.float64)
    g_dev = recover_grad(after["m"], before["m"], cfg.betas[0], 1.0) + gbuf
    for v in views:
        ref = coef * mean[v.name].reshape(-1)
        got = g_dev[v.offset:v.end]
        rn = ref.norm().item()
        if rn == 0.0:
            R.append(Row(k, "grad.zero", v.name, got.norm().item(), 0.0))
            continue
        parts = [g.norm().item() for g in G[v.name].values()]
        R.append(Row(k, "pre.no_cancel", v.name, max(parts) / (rn / coef * cfg.world), NO_CANCEL))
        R.append(Row(k, "pre.m_over_g", v.name, before["m"][v.offset:v.end].double().norm().item() / rn, M_OVER_G))
        tol = TOL_F32_STORAGE if cfg.f32 else (TOL_F32 if v.kernel else TOL_CAST)
        R.append(Row(k, "grad.kernel" if v.kernel else "grad.hooked", v.name, rel(got, ref), tol))

    # ---- the padding behind every parameter stays exactly 0
    for v in views:
        if v.padded_end > v.end:
            bad = sum(float((t[v.end:v.padded_end] != 0).sum()) for t in (g_dev, after["m"], after["v"], after["master"]))
            R.append(Row(k, "pad", v.name, bad, 0.0))

    # ---- master against fp64 AdamW on the snapshot and the recovered gradient, bias correction of step k, decay by the HF rule
    for v in views:
        lo, hi = v.offset, v.end
        p_ref, _, _ = adamw_fp64(before["master"][lo:hi], before["m"][lo:hi], before["v"][lo:hi], g_dev[lo:hi], k, cfg.lr, cfg.betas, cfg.eps,
                                 cfg.weight_decay if v.decay else 0.0)
        R.append(Row(k, "master", v.name, rel(after["master"][lo:hi], p_ref), TOL_ADAMW))

    # ---- state
    R.append(Row(k, "state.work", "work == bf16(master)", float((_bits(after["work"]) != _bits(after["master"].to(torch.bfloat16))).sum()), 0.0))
    work = after["work"]
    for name_B, names_A, BwT, AT in after.get("shadows", ()):
        vb = by[name_B]
        Bw = work[vb.offset:vb.end].view(vb.shape)
        r = Bw.shape[1]
        bad = float((_bits(BwT[:r]) != _bits(Bw.t())).sum()) + float((BwT[r:] != 0).sum()) + float((AT[:, :, r:] != 0).sum())
        for m, n in enumerate(names_A):
            va = by[n]
            bad += float((_bits(AT[m, :, :r]) != _bits(work[va.offset:va.end].view(va.shape).t())).sum())
        R.append(Row(k, "state.shadow", name_B.rsplit(".lora_B", 1)[0], bad, 0.0))
    if after.get("grad") is not None:
        g = after["grad"]
        R.append(Row(k, "state.grad_left_zero", "gradient buffer", float((g != 0).sum()) + float(torch.isnan(g).sum()), 0.0))
    if after.get("t") is not None:
        R.append(Row(k, "state.t", "opt.t", float(abs(after["t"] - k)), 0.0))
    if after.get("grads_set") is not None:
        R.append(Row(k, "state.grad_none", "parameters with .grad set", float(after["grads_set"]), 0.0))
    return R


# ======================================================================================================================================
# a correct step, emulated on the CPU in fp64 / fp32 on a 2-projection layout -- and the ways it can be made wrong
# ======================================================================================================================================
FAULTS = ("micro_batch_missing", "sum_not_mean", "clip_from_sum_norm", "clip_not_clamped", "clip_kernel_fed_only", "decay_on_norm",
          "decay_ignores_padding", "dA1_in_dA2", "stale_AT", "work_truncated", "bias_correction_lags")


class ToyTrainer:
    """Two adapted projections p0 / p1 fed by the same x (one group call per micro-batch), a projector weight and bias and a norm weight as
    hooked parameters (random bf16 gradients per micro-batch); flat fp32 gradient, fused AdamW, bf16 working copy, weight shadows."""
    R, RP, D_IN, M = 4, 8, 15, 3
    D_OUT = (24, 10)

    def __init__(self, cfg: StepCfg, n_micro: int = 2, fault: Optional[str] = None, seed: int = 5):
        assert fault is None or fault in FAULTS
        self.cfg, self.n_micro, self.fault, self.k = cfg, n_micro, fault, 0
        self.gen = torch.Generator().manual_seed(seed)
        shapes = [("proj.weight", (15, 5), False, True), ("proj.bias", (15,), False, False), ("norm.weight", (12,), False, False)]
        for g, do in enumerate(self.D_OUT):
            shapes += [("p%d.lora_A%d.weight" % (g, m), (self.R, self.D_IN), True, True) for m in range(self.M)]
            shapes += [("p%d.lora_B0.weight" % g, (do, self.R), True, True)]
        self.views, off = [], 0
        for n, sh, kernel, decay in shapes:
            sz = math.prod(sh)
            self.views.append(View(n, off, sz, sh, kernel, decay, False))
            off += (sz + 7) // 8 * 8
        self.n = off
        self.master = torch.zeros(off, dtype=torch.float32)
        for v in self.views:
            std = 1.0 if v.name == "norm.weight" else (1.0 / math.sqrt(self.D_IN) if "lora_A" in v.name else 0.2)
            self.master[v.offset:v.end] = (torch.randn(v.size, generator=self.gen) * std).to(torch.bfloat16).float()
        self.m, self.v = torch.zeros(off), torch.zeros(off)
        self.work = self.master.to(torch.bfloat16)
        self.W = [(torch.randn(do, self.D_IN, generator=self.gen) * 0.2).to(torch.bfloat16) for do in self.D_OUT]
        self.hook_dir = {v.name: torch.randn(v.shape, generator=self.gen) * 0.05 for v in self.views if not v.kernel}
        self.shadows = self._make_shadows(None)
        tok = torch.zeros(2, 12, dtype=torch.int64)
        tok[:, 0:4], tok[:, 4:7] = 1, 2
        q = torch.zeros(2, 12, dtype=torch.int64)
        q[0, 8:11], q[1, 7:12] = 1, 1
        self.routing = O.routing_from_avt_masks([(tok == i).long().unsqueeze(-1) for i in range(3)] + [q.unsqueeze(-1)])
        self.spec = SpecRec(self.R, 2.0, (1.0, 1.0, 1.0), 1.0, 1.0 / math.sqrt(self.R), 0.0, 0)

    def _view(self, buf, name):
        v = next(v for v in self.views if v.name == name)
        return buf[v.offset:v.end].view(v.shape)

    def _make_shadows(self, prev):
        out = []
        for g, do in enumerate(self.D_OUT):
            nB, nA = "p%d.lora_B0.weight" % g, ["p%d.lora_A%d.weight" % (g, m) for m in range(self.M)]
            BwT = torch.zeros(self.RP, do, dtype=torch.bfloat16)
            BwT[:self.R] = self._view(self.work, nB).t()
            AT = torch.zeros(self.M, self.D_IN, self.RP, dtype=torch.bfloat16)
            for m, n in enumerate(nA):
                AT[m, :, :self.R] = self._view(self.work, n).t()
            if self.fault == "stale_AT" and prev is not None:
                AT = prev[g][3]
            out.append((nB, nA, BwT, AT))
        return out

    def snapshot(self, with_grad=False):
        s = dict(master=self.master.clone(), m=self.m.clone(), v=self.v.clone(), work=self.work.clone(), t=self.k, grads_set=0,
                 shadows=[(a, b, c.clone(), d.clone()) for a, b, c, d in self.shadows])
        if with_grad:
            s["grad"] = torch.zeros(self.n)
        return s

    def step(self):
        """One step.  Returns (calls, hooked, before, after, returned_norm): what compare_step takes."""
        cfg, f = self.cfg, self.fault
        before = self.snapshot()
        self.k += 1
        k = self.k
        flat = torch.zeros(self.n, dtype=torch.float32)
        calls, hooked = [], {n: [] for n in self.hook_dir}
        n_all = self.n_micro * cfg.world                              # (the micro-batches of every rank add into the sum the ranks share)
        for i in range(n_all):
            x = torch.randn(2, 12, self.D_IN, generator=self.gen).to(torch.bfloat16)
            members, dx = [], torch.zeros(2, 12, self.D_IN, dtype=torch.float64)
            for g, do in enumerate(self.D_OUT):
                nB, nA = "p%d.lora_B0.weight" % g, ["p%d.lora_A%d.weight" % (g, m) for m in range(self.M)]
                gy = (torch.randn(2, 12, do, generator=self.gen) / self.n_micro).to(torch.bfloat16)
                A, Bw = [self._view(self.work, n).double() for n in nA], self._view(self.work, nB).double()
                y0 = x.double() @ self.W[g].double().t()
                y, ctx = O.adapter_forward(x.double(), y0, A, Bw, self.routing, 2.0, [1.0] * 3, 1.0, self.R)
                _, _, BwT, AT = self.shadows[g]
                ctx.A = [AT[m, :, :self.R].t().double() for m in range(self.M)]      # (the input gradient reads the shadows, as the kernels do)
                ctx.Bw = BwT[:self.R].t().double()
                dxa, dA, dB, _ = O.adapter_backward(gy.double(), ctx)
                dx += dxa + gy.double() @ self.W[g].double()
                members.append(Member(nB, nA, self.W[g], None, self.spec, y=y.to(torch.bfloat16), gy=gy))
                if f == "micro_batch_missing" and i == 1:
                    continue
                for m, n in enumerate(nA):
                    dst = nA[{1: 2, 2: 1}.get(m, m)] if (f == "dA1_in_dA2" and g == 0) else n
                    self._view(flat, dst).add_(dA[m].float())
                self._view(flat, nB).add_(dB.float())
            calls.append(Call(i, x, members, gx=dx.to(torch.bfloat16), routing=self.routing))
            for n, d in self.hook_dir.items():
                g_ = ((d + 0.3 * torch.randn(d.shape, generator=self.gen) * 0.05) / self.n_micro).to(torch.bfloat16)
                hooked[n].append(g_)
                if not (f == "micro_batch_missing" and i == 1):
                    self._view(flat, n).add_(g_.float())
        scale = 1.0 if f == "sum_not_mean" else 1.0 / cfg.world
        ret, coef = None, 1.0
        if cfg.max_grad_norm is not None:
            ret = float(flat.norm()) * scale
            nrm = float(flat.norm()) if f == "clip_from_sum_norm" else ret
            coef = cfg.max_grad_norm / (nrm + 1e-6)
            if f != "clip_not_clamped":
                coef = min(1.0, coef)
        sc = torch.full((self.n,), scale * coef, dtype=torch.float64)
        wd = torch.zeros(self.n, dtype=torch.float64)
        unpadded = 0
        for v in self.views:
            if f == "clip_kernel_fed_only" and not v.kernel:
                sc[v.offset:v.padded_end] = scale
            decays = v.decay or (f == "decay_on_norm" and v.name == "norm.weight")
            if f == "decay_ignores_padding":
                wd[unpadded:unpadded + v.size] = cfg.weight_decay if decays else 0.0
                unpadded += v.size
            elif decays:
                wd[v.offset:v.padded_end] = cfg.weight_decay
        t = k - 1 if (f == "bias_correction_lags" and k > 1) else k
        b1, b2 = cfg.betas
        g = flat.double() * sc
        p = self.master.double() * (1.0 - cfg.lr * wd)
        m = b1 * self.m.double() + (1.0 - b1) * g
        v2 = b2 * self.v.double() + (1.0 - b2) * g * g
        p = p - (cfg.lr / (1.0 - b1 ** t)) * (m / (v2.sqrt() / math.sqrt(1.0 - b2 ** t) + cfg.eps))
        self.master, self.m, self.v = p.float(), m.float(), v2.float()
        if f == "work_truncated":
            self.work = (self.master.view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)
        else:
            self.work = self.master.to(torch.bfloat16)
        self.shadows = self._make_shadows(self.shadows)
        return calls, hooked, before, self.snapshot(with_grad=True), ret

    def run(self, K: int = 3) -> List[Row]:
        rows = []
        for _ in range(K):
            calls, hooked, before, after, ret = self.step()
            rows += compare_step(self.views, self.cfg, self.k, calls, hooked, before, after, ret)
        return rows


# ======================================================================================================================================
# the model under test
# ======================================================================================================================================
def _dims(n_kv_heads: int = 2):
    from moka_amd.decoder import LlamaDims
    return LlamaDims(hidden=128, ff=352, n_heads=4, n_kv_heads=n_kv_heads)


def _checkpointed_stack_cls():
    from torch.utils.checkpoint import checkpoint
    from moka_amd.decoder import MokaLlamaStack, rotary_tables

    class CheckpointedStack(MokaLlamaStack):
        def forward(self, h, *mask_args, kv_caches=None, grouped=True, on_layer=None):
            cos, sin = rotary_tables(h.shape[1], self.dims.head_dim, self.dims.rope_theta, h.device, h.dtype)
            for layer in self.layers:
                h = checkpoint(lambda *a, layer=layer: layer.__call__(*a, grouped=grouped)[0], h, cos, sin, *mask_args, use_reentrant=False)
            return h, None
    return CheckpointedStack


class TrainerLM(nn.Module):
    """projector -> MokaLlamaStack of 2 layers -> frozen head, MSE loss.  Trainable: every adapter matrix, the projector's weight and bias,
    both RMSNorm weights of layer 1 (hooked parameters without decay, between the projector and the adapters in the flat buffers)."""

    def __init__(self, dev="cpu", dtype=torch.bfloat16, variant="avt", rank=8, lora_dropout=0.0, checkpoint=False, n_kv_heads=2, seed=13):
        super().__init__()
        from moka_amd.decoder import MokaLlamaStack
        self.dims, self.variant, self.rank = _dims(n_kv_heads), variant, rank
        torch.manual_seed(seed)
        sB = std_B(rank)
        if variant == "avt":
            from moka_amd.peft_hyper import Linear

            def make(d_in, d_out):
                m = Linear(d_in, d_out, r=(rank,) * 3, lora_alpha=ALPHA, lora_nums=3, blc_weight=1.0, blc_alpha=1, lora_dropout=lora_dropout,
                           loramethod="train", bias=False)
                nn.init.normal_(m.weight, std=STD_W)
                nn.init.normal_(m.lora_B0.weight, std=sB)
                return m
        else:
            from moka_amd.modified_peft import Linear as VTLinear

            def make(d_in, d_out):
                base = nn.Linear(d_in, d_out, bias=False)
                nn.init.normal_(base.weight, std=STD_W)
                m = VTLinear(base, "image", r=rank, lora_alpha=ALPHA, lora_dropout=lora_dropout, attn_weight=0.05)
                m.update_layer("text", rank, lora_alpha=ALPHA, lora_dropout=lora_dropout, init_lora_weights=True, use_rslora=False)
                m.set_adapter(["image", "text"])
                for n in ("image", "text"):
                    nn.init.normal_(m.lora_B[n].weight, std=sB)
                return m
        self.vl_projector = nn.Linear(FEAT, self.dims.hidden)
        self.model = (_checkpointed_stack_cls() if checkpoint else MokaLlamaStack)(self.dims, 2, make)
        self.head = nn.Linear(self.dims.hidden, OUT)
        self.to(dev, dtype).train()
        for n, p in self.named_parameters():
            p.requires_grad = ("lora_" in n) or n.startswith("vl_projector") or (n.startswith("model.layers.1.") and "layernorm" in n)

    def forward(self, feats, target, m_t, m_v, m_a, m_q):
        h = self.vl_projector(feats)
        if self.variant == "vt":
            out, _ = self.model(h, m_t.squeeze(-1) == 1, m_v.squeeze(-1) == 1, m_q.squeeze(-1) == 1)
        else:
            out, _ = self.model(h, [m_t, m_v, m_a, m_q])
        return {"loss": (self.head(out).float() - target.float()).square().mean()}


def make_batch(seed: int, shift: int = 0, no_image_sample: Optional[int] = None, B: int = B_, S: int = S_, dtype=torch.bfloat16) -> dict:
    """Modality and question spans that differ per sample and move with `shift`; the last sample's question span touches the end of the
    sequence (its length changes with `shift`).  no_image_sample: that sample has no video / image token."""
    g = torch.Generator().manual_seed(1000 + seed)
    tok = torch.zeros(B, S, dtype=torch.int64)
    q = torch.zeros(B, S, dtype=torch.bool)
    for b in range(B):
        if b != no_image_sample:
            tok[b, 4 + 2 * b + shift:20 + 3 * b + shift] = 1
        tok[b, 24 + b + shift:36 + 2 * b + shift] = 2
        if b == B - 1:
            q[b, S - 14 - 2 * shift:] = True
        else:
            q[b, 44 + 4 * b + shift:54 + 10 * b + 3 * shift] = True
    assert not (q & (tok != 0)).any()
    out = {"feats": torch.randn(B, S, FEAT, generator=g).to(dtype), "target": torch.randn(B, S, OUT, generator=g)}
    for key, m in (("m_t", 0), ("m_v", 1), ("m_a", 2)):
        out[key] = (tok == m).to(torch.int32).unsqueeze(-1)
    out["m_q"] = q.to(torch.int32).unsqueeze(-1)
    return out


def oracle_routing(variant: str, batch: dict):
    m = {k: batch[k].cpu() for k in ("m_t", "m_v", "m_a", "m_q")}
    if variant == "vt":
        return O.routing_from_vt_masks(m["m_t"].squeeze(-1) == 1, m["m_v"].squeeze(-1) == 1, m["m_q"].squeeze(-1) == 1)
    return O.routing_from_avt_masks([m["m_t"], m["m_v"], m["m_a"], m["m_q"]])


# ---- the whole model in fp64 on the CPU: what the scales and the clip thresholds are chosen from (no kernel, no dropout)
def _adapter_parts(mod):
    if hasattr(mod, "lora_B0"):
        return (mod.weight, [getattr(mod, "lora_A%d" % i).weight for i in range(mod.lora_num)], mod.lora_B0.weight, mod.scaling[0],
                [1.0] * mod.lora_num, mod.blc_weight, mod.d_k)
    r = mod.r["text"]
    return (mod.get_base_layer().weight, [mod.lora_A["text"].weight, mod.lora_A["image"].weight], mod.lora_B["text"].weight, 1.0,
            [mod.scaling["text"], mod.scaling["image"]], mod.attn_weight, r)


def reference_loss(model: TrainerLM, batch: dict, ratios: Optional[list] = None):
    """(loss, params): the model's loss in fp64 through plain torch ops and O.adapter_forward; params[name] = the fp64 leaf of every
    trainable parameter (torch.autograd.grad on them gives the reference gradient).  ratios: gets |adapter term| / |base term| per call."""
    from moka_amd.decoder import _rotate, rotary_tables
    f64 = torch.float64
    params = {n: p.detach().to(f64).requires_grad_(True) for n, p in model.named_parameters() if p.requires_grad}
    ids = {id(p): n for n, p in model.named_parameters()}
    W = lambda p: params[ids[id(p)]] if ids[id(p)] in params else p.detach().to(f64)          # noqa: E731
    ort = oracle_routing(model.variant, batch)
    d = model.dims

    def proj(mod, x):
        Wb, A, Bw, s_in, s_out, w, d_k = _adapter_parts(mod)
        y0 = x @ W(Wb).t()
        y, _ = O.adapter_forward(x, y0, [W(a) for a in A], W(Bw), ort, s_in, s_out, w, d_k)
        if ratios is not None:
            ratios.append(((y - y0).norm() / y0.norm()).item())
        return y

    def rms(x, mod):
        return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + (mod.eps if mod.eps is not None else torch.finfo(f64).eps)) * W(mod.weight)

    feats = batch["feats"].cpu().to(f64)
    Bn, Sn = feats.shape[:2]
    h = feats @ W(model.vl_projector.weight).t() + W(model.vl_projector.bias)
    cos, sin = rotary_tables(Sn, d.head_dim, d.rope_theta, "cpu", f64)
    for layer in model.model.layers:
        a = layer.self_attn
        x = rms(h, layer.input_layernorm)
        q, k_, v = proj(a.q_proj, x), proj(a.k_proj, x), proj(a.v_proj, x)
        q = _rotate(q.view(Bn, Sn, d.n_heads, d.head_dim).transpose(1, 2), cos, sin)
        k_ = _rotate(k_.view(Bn, Sn, d.n_kv_heads, d.head_dim).transpose(1, 2), cos, sin)
        v = v.view(Bn, Sn, d.n_kv_heads, d.head_dim).transpose(1, 2)
        rep = d.n_heads // d.n_kv_heads
        k_, v = k_.repeat_interleave(rep, dim=1), v.repeat_interleave(rep, dim=1)
        o = torch.nn.functional.scaled_dot_product_attention(q, k_, v, is_causal=True).transpose(1, 2).reshape(Bn, Sn, -1)
        h = h + proj(a.o_proj, o)
        x = rms(h, layer.post_attention_layernorm)
        h = h + proj(layer.mlp.down_proj, torch.nn.functional.silu(proj(layer.mlp.gate_proj, x)) * proj(layer.mlp.up_proj, x))
    out = h @ W(model.head.weight).t() + W(model.head.bias)
    return (out - batch["target"].cpu().to(f64)).pow(2).mean(), params


# ======================================================================================================================================
# the GPU half: the record and the run
# ======================================================================================================================================
class _DevCall:
    def __init__(self, micro, x, rt, gen, capturing):
        self.micro, self.x, self.rt, self.gen, self.capturing = micro, x, rt, gen, capturing
        self.gx, self.members = [], []


class Recorder:
    """Wraps moka_linear / moka_linear_group where the layers look them up.  Everything stays on the device until ``calls()`` (the wrapper
    runs inside stream captures too: its clones become copies inside the graph that every replay refreshes)."""

    def __init__(self, model: nn.Module):
        self.name_of = {id(p): n for n, p in model.named_parameters()}
        self.model = model
        self.records: List[_DevCall] = []
        self.hooked: List[tuple] = []               # (name, micro, gen, capturing, gradient)
        self.micro, self.gen = 0, 0
        self._handles = []

    def install(self, monkeypatch, hooked_names: Sequence[str]):
        dec = importlib.import_module("moka_amd.decoder")
        for path in ("moka_amd.peft_hyper.lora", "moka_amd.modified_peft.layer"):
            mod = importlib.import_module(path)
            monkeypatch.setattr(mod, "moka_linear", self._single(mod.moka_linear))
        monkeypatch.setattr(dec, "moka_linear_group", self._group(dec.moka_linear_group))
        by = dict(self.model.named_parameters())
        for n in hooked_names:
            self._handles.append(by[n].register_hook(lambda g, n=n: self.hooked.append(
                (n, self.micro, self.gen, bool(torch.cuda.is_current_stream_capturing()), g.detach().clone()))))

    def remove(self):
        for h in self._handles:
            h.remove()

    def reset(self):
        self.records, self.hooked = [], []

    def _begin(self, x, rt, projections, specs):
        c = _DevCall(self.micro, x.detach().clone(), rt, self.gen, bool(torch.cuda.is_current_stream_capturing()))
        for (W, bias, Bw, A), sp in zip(projections, specs):
            mb = Member(self.name_of[id(Bw)], [self.name_of[id(a)] for a in A], W, bias,
                        SpecRec(sp.r, sp.s_in, tuple(sp.s_out), sp.w, sp.inv_sqrt_dk, sp.dropout_p, sp.seed))
            mb.gy = []
            c.members.append(mb)
        if x.requires_grad:
            x.register_hook(lambda g, c=c: c.gx.append(g.detach().clone()))
        self.records.append(c)
        return c

    def _end(self, c, ys):
        for mb, y in zip(c.members, ys):
            mb.y = y.detach().clone()
            if y.requires_grad:
                y.register_hook(lambda g, mb=mb: mb.gy.append(g.detach().clone()))

    def _single(self, orig):
        def moka_linear(x, W, bias, Bw, A, rt, spec):
            c = self._begin(x, rt, [(W, bias, Bw, A)], [spec])
            y = orig(x, W, bias, Bw, A, rt, spec)
            self._end(c, [y])
            return y
        return moka_linear

    def _group(self, orig):
        def moka_linear_group(x, projections, rt, specs):
            c = self._begin(x, rt, projections, specs)
            ys = orig(x, projections, rt, specs)
            self._end(c, ys)
            return ys
        return moka_linear_group

    def calls(self, routings: Sequence, epoch: int, pick=lambda c: True) -> List[Call]:
        """The records as CPU calls (after a synchronize).  routings[micro] = the oracle routing; epoch: dp.seed_epoch of the step."""
        from moka_amd import _lib
        from moka_amd import functional as F
        out = []
        for c in self.records:
            if not pick(c):
                continue
            x = c.x.cpu()
            Bc, Sc = x.shape[0], x.shape[1]
            members = []
            for mb in c.members:
                assert len(mb.gy) <= 1 and len(c.gx) <= 1, "a gradient hook fired more than once"
                keep, inv = None, 1.0
                if mb.spec.dropout_p > 0:
                    keep = F.dropout_mask(mb.spec.dropout_p, F.effective_seed(mb.spec.seed, epoch), Bc * Sc, x.shape[-1], c.x.device)
                    keep = keep.cpu().double().reshape(Bc, Sc, -1)
                    inv = float(_lib.load().moka_dropout_scale(float(mb.spec.dropout_p)))
                members.append(Member(mb.name_B, mb.names_A, mb.W.detach().cpu(), None if mb.bias is None else mb.bias.detach().cpu(), mb.spec,
                                      y=None if mb.y is None else mb.y.cpu(), gy=mb.gy[0].cpu() if mb.gy else None, keep=keep, inv_keep=inv))
            out.append(Call(c.micro, x, members, gx=c.gx[0].cpu() if c.gx else None, routing=routings[c.micro]))
        return out

    def hooked_grads(self, names: Sequence[str], n_micro: int, pick=lambda gen, capturing: True) -> Dict[str, List[torch.Tensor]]:
        out = {n: [None] * n_micro for n in names}
        for n, micro, gen, cap, g in self.hooked:
            if pick(gen, cap):
                assert out[n][micro] is None, "%s: two gradients in one micro-batch" % n
                out[n][micro] = g.cpu()
        return {n: [g for g in gs if g is not None] for n, gs in out.items()}


class Config(NamedTuple):
    variant: str = "avt"
    rank: int = 8
    dtype: torch.dtype = torch.bfloat16
    n_micro: int = 1
    defer_dA: bool = True
    dropout: float = 0.0
    max_grad_norm: Optional[float] = None
    clip_expect: Optional[str] = None
    weight_decay: float = 0.01
    opt_in_backward: bool = False
    n_buckets: int = 2
    persistent_shadows: Optional[bool] = None
    checkpoint: bool = False
    n_kv_heads: int = 2
    graph_chains: int = 0                       # > 0: schedule.GraphedTrainStep with that many chains
    lr: float = 2e-3


class TrainerRun:
    """K optimizer steps of TrainerLM under attach(), each checked by compare_step."""

    def __init__(self, cfg: Config, monkeypatch):
        from moka_amd.parallel import attach
        assert torch.cuda.is_available(), "the trainer step has no CPU path"
        self.cfg, self.dev = cfg, torch.device("cuda", 0)
        self.model = TrainerLM(self.dev, cfg.dtype, cfg.variant, cfg.rank, cfg.dropout, cfg.checkpoint, cfg.n_kv_heads)
        self.views = expected_layout(self.model)
        self.dp = dp = attach(self.model, n_buckets=cfg.n_buckets, lr=cfg.lr, weight_decay=cfg.weight_decay, defer_dA=cfg.defer_dA,
                              optimizer_in_backward=cfg.opt_in_backward, persistent_shadows=cfg.persistent_shadows)
        assert [(v.name, v.offset, v.size) for v in self.views] == list(zip(dp.names, dp.offsets, dp.sizes)), "attach() laid the parameters out differently"
        assert {v.name for v in self.views if v.kernel} == set(dp.kernel_fed)
        self.rec = Recorder(self.model)
        self.rec.install(monkeypatch, dp.hooked)
        # how many problems left through the per-layer batched launches _flush_deferred builds (counted, nothing else)
        from moka_amd import functional as F
        self.batched = {"da": 0, "db": 0}
        for kind, fn_name in (("da", "down_bwd_da_batch_"), ("db", "up_bwd_db_batch_")):
            def counting(first, *a, _orig=getattr(F, fn_name), _kind=kind, **kw):
                self.batched[_kind] += len(first)
                return _orig(first, *a, **kw)
            monkeypatch.setattr(F, fn_name, counting)
        self.step_cfg = StepCfg(lr=cfg.lr, weight_decay=cfg.weight_decay, world=1, f32=cfg.dtype == torch.float32,
                                max_grad_norm=None if cfg.opt_in_backward else cfg.max_grad_norm, clip_expect=cfg.clip_expect)
        self.report: List[Row] = []
        self.k = 0
        self.gs, self.capture_error = None, None
        if cfg.graph_chains:
            self._capture()

    # ---------------------------------------------------------------------------------------------------- batches
    def batch(self, k: int, i: int = 0) -> dict:
        """Micro-batch i of step k (k = 0: the example a captured step is built on).  The spans move with the step and the micro-batch; in the
        VT configuration sample 1 has no image token."""
        shift = {0: 0, 1: 2, 2: 0, 3: 3}[k] + i
        b = make_batch(10 * k + i, shift, no_image_sample=1 if self.cfg.variant == "vt" else None, dtype=self.cfg.dtype)
        return {n: t.to(self.dev) for n, t in b.items()}

    def _routing_fn(self, part):
        from moka_amd.routing import MokaRouting
        return MokaRouting.from_avt_masks([part["m_t"], part["m_v"], part["m_a"], part["m_q"]])

    def _capture(self):
        from moka_amd import schedule as SCH
        cfg, rec = self.cfg, self.rec
        count, gen_of = [0], {}
        once = SCH.GraphedTrainStep._capture_once

        def capture_once(gs):
            rec.gen += 1
            out = once(gs)
            gen_of[id(out[0])] = rec.gen
            return out

        def step_fn(part):
            rec.micro = count[0] % cfg.graph_chains
            count[0] += 1
            return self.model(**part)["loss"]
        SCH.GraphedTrainStep._capture_once = capture_once
        try:
            self.gs = SCH.GraphedTrainStep(self.dp, step_fn, self.batch(0), chains=cfg.graph_chains, routing_fn=self._routing_fn)
        finally:
            SCH.GraphedTrainStep._capture_once = once
        gen = gen_of[id(self.gs.graph)]
        self.rec.records = [c for c in rec.records if c.capturing and c.gen == gen]       # (kept alive: the graph's replays write into them)
        self.rec.hooked = [h for h in rec.hooked if h[3] and h[2] == gen]
        self.sizes = list(self.gs.sizes)

    # ---------------------------------------------------------------------------------------------------- state
    def _snapshot(self, with_grad=False) -> dict:
        dp, o = self.dp, self.dp.optimizer
        s = dict(master=dp.master.detach().cpu().clone(), m=o.exp_avg.cpu().clone(), v=o.exp_avg_sq.cpu().clone(), work=dp.work.detach().cpu().clone(),
                 t=o.t, shadows=[(self.rec.name_of[id(Bw)], [self.rec.name_of[id(a)] for a in As], BwT.cpu().clone(), AT.cpu().clone())
                                 for _, _, Bw, As, BwT, AT in dp._shadowed])
        if with_grad:
            s["grad"] = dp.bucket.flat.cpu().clone()
            s["grads_set"] = sum(p.grad is not None for p in self.model.parameters())
        return s

    # ---------------------------------------------------------------------------------------------------- one step
    def step(self):
        import warnings
        cfg, dp, rec = self.cfg, self.dp, self.rec
        before = self._snapshot()
        self.k += 1
        k = self.k
        ret = None
        if self.gs is not None:
            full = self.batch(k)
            parts = [{n: t[lo:lo + sz] for n, t in full.items()} for lo, sz in zip([sum(self.sizes[:c]) for c in range(len(self.sizes))], self.sizes)]
            self.gs(full)
        else:
            rec.reset()
            parts = [self.batch(k, i) for i in range(cfg.n_micro)]
            for i, part in enumerate(parts):
                rec.micro = i
                with (dp.no_sync() if i < cfg.n_micro - 1 else contextlib.nullcontext()):
                    (self.model(**part)["loss"] / cfg.n_micro).backward()
            if cfg.opt_in_backward:
                with warnings.catch_warnings(record=True) as caught:
                    warnings.simplefilter("always")
                    ret = dp.step(max_grad_norm=cfg.max_grad_norm)
                n_warn = sum(issubclass(w.category, RuntimeWarning) and "does NOT clip" in str(w.message) for w in caught)
                self.report.append(Row(k, "state.unclipped", "RuntimeWarning per step, unclipped_steps == k, nothing returned",
                                       float(n_warn != 1) + float(dp.unclipped_steps != k) + float(ret is not None), 0.0))
                ret = None
            else:
                ret = dp.step(max_grad_norm=cfg.max_grad_norm)
        torch.cuda.synchronize()
        ret = None if ret is None else float(ret)
        epoch = int(dp.seed_epoch.item())
        after = self._snapshot(with_grad=True)
        routings = [oracle_routing(cfg.variant, p) for p in parts]
        calls = rec.calls(routings, epoch)
        seen = set()
        for c_dev in rec.records:                                        # the device routing against the oracle's, once per batch
            if c_dev.micro not in seen:
                seen.add(c_dev.micro)
                _check_routing(c_dev.rt, routings[c_dev.micro])
        hooked = rec.hooked_grads(dp.hooked, len(parts))
        self.n_calls = len(calls)
        if cfg.checkpoint:                                               # every call is recorded twice: the forward and its re-forward
            n_re = sum(c.is_reforward for c in calls)
            self.report.append(Row(k, "ckpt.twice", "%d calls, %d re-forwards" % (len(calls) - n_re, n_re), float(abs(len(calls) - 2 * n_re)), 0.0))
        self.report += compare_step(self.views, self.step_cfg, k, calls, hooked, before, after, ret)

    def run(self, K: int = 3) -> List[Row]:
        try:
            for _ in range(K):
                self.step()
        finally:
            self.rec.remove()
            self.dp.detach()
        return self.report


def preconditions(report: Sequence[Row]) -> str:
    return "; ".join("%s %.3g / %.3g (step %d, %s)" % (c, r.value, r.bound, r.step, r.where) for c, r in sorted(worst(report).items())
                     if c.startswith("pre."))
