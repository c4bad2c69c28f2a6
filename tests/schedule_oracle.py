"""The benchmarked training step against the fp64 oracle (a helper module like ``tests/arena.py``, not a conftest).

``bench.py`` times ``moka_amd.schedule.GraphedAdapterStep`` over the workload ``bench.build_workload`` lays out.  That path drives the C
ABI through its own pre-built ctypes argument lists (``AdapterUnit.calls`` / ``da_items`` / ``sh_items`` / ``db_items``,
``make_layer_batches``, ``run_shadows``' cached batches); ``bench.py --verify-graph`` compares it with the same lists launched live, i.e.
with itself.  This harness runs K real steps of the real executor on a small workload built by the real ``build_workload``, snapshots the
caller-owned buffers in front of every step, recomputes the step with ``oracle/moka_oracle.py`` in fp64 and compares everything the step
leaves behind: y, dx, the gradient of every parameter view, the fp32 master after the AdamW slice, the bf16 working copy, the weight
shadows, the step counters and the dropout epochs.

What the harness does to the workload, and why:

* the y / dx buffers ``build_workload`` fills with N(0, 1) are scaled by a power of two (exact in bf16, touches nothing else), chosen
  from the oracle alone so that the adapter term is about as large as the base it is added to -- unscaled it sits below one bf16 ulp of
  the base and no element-wise check would see it.  Asserted per buffer and pass: 0.25 <= |term| / |base| <= 4;
* ``GraphedAdapterStep.capture()`` runs the step's launches once as a warm-up, which is not a step.  The harness captures with
  ``restore_grad=True`` (the flat gradient comes back as it was: step 1's AdamW slices see that step's gradient alone -- without it
  grad.dA / grad.dB are 0.73 - 0.95 off at step 1) and does not touch the gradient itself, so step 1 checks exactly that; it puts the
  warm-up's additions to y / dx back, so that step 1 starts from the scaled buffers like every other step.

``bench_exact=True``: no scaling, a plain ``capture()``, nothing put back -- exactly the launches ``bench.main`` makes (test h ties that to
the real entry point).  The y / dx rows then cannot see the adapter term (below a bf16 ulp of the N(0, 1) base) and the term / base
precondition is not evaluated: the gradient and state rows carry the weight there.

Tolerances are the project's own: ``TOL_BF16`` / ``TOL_F32`` / ``ulp_bf16_diff`` of ``tests/test_gpu_parity.py``, 2e-6 of
``tests/test_gpu_parallel.py`` (the fused AdamW against the torch formula).  The pure parts (fp64 AdamW, gradient recovery from two
first moments, the pass counter, the report) need no GPU: ``tests/test_schedule_oracle_host.py``.
"""
from __future__ import annotations

import importlib
import math
import os
import sys
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import moka_oracle as O  # noqa: E402
from tests.test_gpu_parity import TOL_BF16, TOL_F32, ulp_bf16_diff  # noqa: E402

TOL_ADAMW = 2e-6                # tests/test_gpu_parallel.py: moka_adamw_flat against the torch formula, relative, per parameter tensor
M_OVER_G = 2.0                  # precondition of the gradient recovery: |m_{k-1}| <= 2 |g| keeps its noise (~5e-7 |m| / |g|) under 2e-6
TERM_LO, TERM_HI = 0.25, 4.0    # precondition of the y / dx checks: |adapter term| / |base|

# tiny widths (multiples of 32; 704 leaves a half-filled wave), injected as bench.MODELS["7b"] so that every `auto` of bench.main resolves
# as it does for the headline: mha -- every unit takes the fused forward; gqa -- q+k+v is a group of unequal d_out (three-launch forward)
WIDTHS = {"mha": dict(d=256, ff=704, kv=256, layers=32), "gqa": dict(d=256, ff=704, kv=64, layers=32)}
BASE_ARGV = ["--gpus", "1", "--seq", "256", "--batch", "3", "--layers", "2", "--distinct", "2"]


class Row(NamedTuple):
    step: int
    check: str
    where: str
    value: float
    bound: float


def failed(row: Row) -> bool:
    """Every check is `value <= bound` (a NaN fails; two-sided conditions are two rows)."""
    return not (row.value <= row.bound)


def failures(report: Sequence[Row], check: Optional[str] = None, step: Optional[int] = None) -> List[Row]:
    return [r for r in report if failed(r) and (check is None or r.check == check or r.check.startswith(check + "."))
            and (step is None or r.step == step)]


def worst(report: Sequence[Row]) -> Dict[str, Row]:
    """The row closest to (or furthest past) its bound, per check."""
    def load(r):
        if not (r.value == r.value):
            return float("inf")
        return r.value / r.bound if r.bound > 0 else (float("inf") if r.value > 0 else 0.0)
    out: Dict[str, Row] = {}
    for r in report:
        if r.check not in out or load(r) > load(out[r.check]):
            out[r.check] = r
    return out


def summary(report: Sequence[Row]) -> str:
    return "; ".join("%s %.3g / %.3g (step %d, %s)" % (c, r.value, r.bound, r.step, r.where) for c, r in sorted(worst(report).items()))


def rel(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.double().cpu(), b.double().cpu()
    n = b.norm().item()
    d = (a - b).norm().item()
    return d / n if n > 0 else d


# ======================================================================================================================================
# pure parts
# ======================================================================================================================================
def adamw_fp64(p, m, v, g, t: int, lr: float, betas, eps: float, weight_decay: float):
    """One step of the torch.optim.AdamW formula in fp64: returns (p, m, v) after step t (1-based)."""
    p, m, v, g = p.double(), m.double(), v.double(), g.double()
    b1, b2 = float(betas[0]), float(betas[1])
    p = p * (1.0 - lr * weight_decay)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    denom = v.sqrt() / math.sqrt(1.0 - b2 ** t) + eps
    return p - (lr / (1.0 - b1 ** t)) * (m / denom), m, v


def f32_beta(beta1: float) -> Tuple[float, float]:
    """(beta1, 1 - beta1) as the kernel holds them: beta1 rounded to fp32, the difference taken in fp32 (k_misc.hip: moka_adamw_kernel)."""
    b = torch.tensor(float(beta1), dtype=torch.float32)
    return float(b.double()), float((torch.tensor(1.0, dtype=torch.float32) - b).double())


def recover_grad(m_new: torch.Tensor, m_old: torch.Tensor, beta1: float, grad_scale: float = 1.0) -> torch.Tensor:
    """The gradient an AdamW slice consumed, from the first moment before and after it: m_k = beta1 m_{k-1} + (1 - beta1) scale g."""
    b1, omb1 = f32_beta(beta1)
    return (m_new.double() - b1 * m_old.double()) / (omb1 * float(grad_scale))


class UnitDesc(NamedTuple):
    """What the pass counter needs of a unit: the activation set it works on, the input it reads, the projections it writes."""
    set: int
    src: str
    members: Tuple[str, ...]


def count_passes(units: Sequence[UnitDesc]):
    """Read-modify-write passes of one step per buffer: y[(set, projection)] is written once by the unit that holds the projection, dx[(set,
    input)] once per unit fed by that input (a group is ONE pass: its members' dx are summed before the store).  Layers that share an
    activation set add."""
    y: Dict[Tuple[int, str], int] = {}
    dx: Dict[Tuple[int, str], int] = {}
    for u in units:
        dx[(u.set, u.src)] = dx.get((u.set, u.src), 0) + 1
        for name in u.members:
            y[(u.set, name)] = y.get((u.set, name), 0) + 1
    return y, dx


# ======================================================================================================================================
# arguments: bench.parse_args + the `auto` resolution of bench.main
# ======================================================================================================================================
def _bench():
    return importlib.import_module("bench")


def resolve_args(argv: Sequence[str]):
    """bench.parse_args(argv) with the `auto` fields resolved EXACTLY as bench.main does (bench.py lines 694-715 and 770: main is monolithic,
    so the lines are repeated here; test h of tests/test_gpu_schedule_oracle.py ties this copy to the real entry point)."""
    bench = _bench()
    from moka_amd import _lib
    args = bench.parse_args(list(argv))
    if args.layers is None:
        args.layers = bench.MODELS[args.model]["layers"]
    if args.graph == "auto":
        args.graph = "all" if (int(os.environ.get("WORLD_SIZE", "1")) == 1 and not args.force_comm) else "bwd"
    if args.chains == 0:
        args.chains = 2 if (args.graph != "off" and args.batch >= 2 and args.model in ("7b", "13b") and args.rank <= 32) else 1
    if args.graph_topology == "auto":
        args.graph_topology = "hub" if args.chains > 1 else "chain"
    if args.defer_da == "auto":
        args.defer_da = "unit" if (args.chains > 1 and args.graph != "off") else "layer"
    args.hub = args.graph != "off" and (args.graph_topology == "hub" or args.chains > 1)
    if args.chain_priority == "auto":
        args.chain_priority = "high" if (args.graph == "all" and args.rank <= 32) else "normal"
    lib = _lib.load()
    args.split_db = args.defer_da != "off" and (args.defer_db == "on" or (args.defer_db == "auto" and lib.moka_up_bwd_passes(args.rank, 0) == 2))
    return args


# ======================================================================================================================================
# the oracle of one step
# ======================================================================================================================================
class Member(NamedTuple):
    name: str
    pi: int
    d_in: int
    d_out: int
    off_A: Tuple[int, ...]      # offsets of A_m / dA_m in the flat buffers
    off_B: int
    seed: int


class UnitPlan(NamedTuple):
    layer: int
    set: int
    src: str
    members: Tuple[Member, ...]
    fused: bool


class ChainPlan(NamedTuple):
    B: int
    S: int
    routing: object             # oracle Routing
    units: Tuple[UnitPlan, ...]


class Plan(NamedTuple):
    chains: Tuple[ChainPlan, ...]
    r: int
    M: int
    n_params: int
    s_in: float
    s_out: Tuple[float, ...]
    w: float
    p: float

    def unit_descs(self) -> List[UnitDesc]:
        return [UnitDesc(u.set, u.src, tuple(m.name for m in u.members)) for u in self.chains[0].units]

    def views(self):
        """(where, lo, hi, kind) of every parameter view of the flat buffers."""
        out = []
        for u in self.chains[0].units:
            for mb in u.members:
                for m, o in enumerate(mb.off_A):
                    out.append(("L%d.%s.dA%d" % (u.layer, mb.name, m), o, o + self.r * mb.d_in, "dA"))
                out.append(("L%d.%s.dB" % (u.layer, mb.name), mb.off_B, mb.off_B + mb.d_out * self.r, "dB"))
        return out


def flat_layout(dims, L: int, r: int, M: int):
    """Offsets of A_m / Bw of (layer, projection) in the flat buffers: the layout bench.build_workload documents (layer-major, the seven
    projections in PROJS order, M adapters [r, d_in] then Bw [d_out, r]), restated here independently of the views it hands the units."""
    bench = _bench()
    off, out = 0, {}
    for l in range(L):
        for pi, (name, di, do, src) in enumerate(bench.PROJS):
            d_in, d_out = dims[di], dims[do]
            oa = []
            for _ in range(M):
                oa.append(off)
                off += r * d_in
            out[(l, pi)] = (tuple(oa), off, d_in, d_out, src, name)
            off += d_out * r
    return out, off


def make_plan(wl, args) -> Plan:
    bench = _bench()
    vt = args.variant == "vt"
    r, M, L = args.rank, (2 if vt else 3), args.layers
    layout, n_params = flat_layout(bench.MODELS[args.model], L, r, M)
    assert n_params == wl["n_params"]
    names = [p[0] for p in bench.PROJS]
    nset = max(1, min(L, args.distinct))
    s = 16.0 / r
    chains = []
    for ci, ch in enumerate(wl["chains"]):
        sets, masks, _, _ = wl["keep"][ci]
        if vt:
            rt = O.routing_from_vt_masks(*[m.cpu() for m in masks])
            Bc, Sc = masks[0].shape
        else:
            rt = O.routing_from_avt_masks([m.cpu() for m in masks])
            Bc, Sc = masks[0].shape[:2]
        assert Bc * Sc == ch["T"]
        per = ch["units_per_layer"]
        units = []
        for ui, u in enumerate(ch["units"]):
            l = ui // per
            si = l % nset
            acts, dacts, ys = sets[si]
            src_ = layout[(l, names.index(u.members[0]["name"]))][4]
            assert u.x.data_ptr() == acts[src_].data_ptr() and u.dx.data_ptr() == dacts[src_].data_ptr(), "unit %d: x / dx of another set or input" % ui
            mem = []
            for g, m in enumerate(u.members):
                pi = names.index(m["name"])
                oa, ob, d_in, d_out, src, _ = layout[(l, pi)]
                mem.append(Member(m["name"], pi, d_in, d_out, oa, ob, u.seeds[g]))
            src = layout[(l, mem[0].pi)][4]
            assert all(layout[(l, mb.pi)][4] == src for mb in mem), "a unit's projections read one input"
            units.append(UnitPlan(l, si, src, tuple(mem), bool(u.fused)))
        chains.append(ChainPlan(int(Bc), int(Sc), rt, tuple(units)))
    return Plan(tuple(chains), r, M, n_params, 1.0 if vt else s, tuple([s] * M if vt else [1.0] * M), 0.05 if vt else 1.0, float(args.dropout))


def oracle_step(plan: Plan, snap: dict, keep_fn, y_after: Optional[dict] = None, rows: Optional[list] = None, step: int = 0):
    """One step in fp64 from the snapshot `snap` (work bf16; acts / y / dx per (chain, set, key)).  keep_fn(ci, member, Tc) -> the member's
    keep mask times 1/(1-p') as a double [Tc, d_in] tensor, or None.  y_after: the device's y after the step, used as gy (stage-wise
    comparison, as tests/test_gpu_parity._stage_check); None: the oracle's own y.  Every read-modify-write pass the schedule makes rounds
    to bf16.  Returns (y, dx, grad, peak): dicts keyed like the snapshot, the flat fp64 gradient summed over chains, and per buffer the largest
    magnitude every element held during the step (the operand of the ulp check).  rows: gets the |term| / |base| precondition of every
    pass (oracle values only)."""
    f64, bf = torch.float64, torch.bfloat16
    work = snap["work"].double()
    grad = torch.zeros(plan.n_params, dtype=f64)
    y_cur = {k: v.double() for k, v in snap["y"].items()}
    dx_cur = {k: v.double() for k, v in snap["dx"].items()}
    # the largest magnitude every element held during the step (the snapshot and the result of every pass): the resolution a buffer that
    # several passes update in place ever had -- a second pass that cancels the first leaves a small value with the first one's ulp
    peak = {"y": {k: v.abs() for k, v in y_cur.items()}, "dx": {k: v.abs() for k, v in dx_cur.items()}}
    r = plan.r

    def pre(kind, where, term, base):
        if rows is not None:
            t, b = term.norm().item(), base.norm().item()
            rows.append(Row(step, "pre.term_over_base", "%s.%s" % (kind, where), t / b if b > 0 else float("inf"), TERM_HI))
            rows.append(Row(step, "pre.base_over_term", "%s.%s" % (kind, where), b / t if t > 0 else float("inf"), 1.0 / TERM_LO))

    for ci, ch in enumerate(plan.chains):
        Bc, Sc, Tc = ch.B, ch.S, ch.B * ch.S
        saved = {}
        for ui, u in enumerate(ch.units):
            x = snap["acts"][(ci, u.set, u.src)].double()
            for mb in u.members:
                keep = keep_fn(ci, mb, Tc)
                xe = x if keep is None else x * keep
                A = [work[o:o + r * mb.d_in].view(r, mb.d_in) for o in mb.off_A]
                Bw = work[mb.off_B:mb.off_B + mb.d_out * r].view(mb.d_out, r)
                key = (ci, u.set, mb.name)
                y0 = y_cur[key]
                y, ctx = O.adapter_forward(xe.reshape(Bc, Sc, -1), y0.reshape(Bc, Sc, -1), A, Bw, ch.routing, plan.s_in, plan.s_out, plan.w, r)
                y = y.reshape(Tc, -1)
                pre("y", "chain%d.set%d.%s.L%d" % (ci, u.set, mb.name, u.layer), y - y0, y0)
                y_cur[key] = y.to(bf).double()
                peak["y"][key] = torch.maximum(peak["y"][key], y_cur[key].abs())
                saved[(ui, mb.name)] = (ctx, keep)
        for ui in range(len(ch.units) - 1, -1, -1):
            u = ch.units[ui]
            tot = None
            for mb in u.members:
                ctx, keep = saved.pop((ui, mb.name))
                key = (ci, u.set, mb.name)
                gy = (y_after[key].double() if y_after is not None else y_cur[key]).reshape(Bc, Sc, -1)
                dxa, dA, dB, _ = O.adapter_backward(gy, ctx)
                dxa = dxa.reshape(Tc, -1)
                if keep is not None:
                    dxa = dxa * keep
                tot = dxa if tot is None else tot + dxa
                for o, g_ in zip(mb.off_A, dA):
                    grad[o:o + r * mb.d_in] += g_.reshape(-1)
                grad[mb.off_B:mb.off_B + mb.d_out * r] += dB.reshape(-1)
            key = (ci, u.set, u.src)
            pre("dx", "chain%d.set%d.%s.L%d" % (ci, u.set, u.src, u.layer), tot, dx_cur[key])
            dx_cur[key] = (dx_cur[key] + tot).to(bf).double()        # a grouped dx is ONE pass
            peak["dx"][key] = torch.maximum(peak["dx"][key], dx_cur[key].abs())
    return y_cur, dx_cur, grad, peak


# ======================================================================================================================================
# the run
# ======================================================================================================================================
class ScheduleRun:
    """K steps of bench's GraphedAdapterStep on bench's workload, each checked against the oracle.  argv: bench.py's command line;
    skip: kernel families left out (negative controls: ScheduleConfig.skip);  bench_exact: no scaling, a plain capture(), nothing put back behind it."""

    def __init__(self, argv: Sequence[str], skip: Sequence[str] = (), bench_exact: bool = False):
        bench = _bench()
        from moka_amd import _lib, schedule as SCH
        from moka_amd.parallel import FlatAdamW, FlatGradBucket, geometric_buckets
        assert torch.cuda.is_available(), "the schedule has no CPU path"
        self.args = args = resolve_args(argv)
        self.dev = dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        self.lib = lib = _lib.load()
        _lib.check(lib.moka_device_check(), "moka_device_check")
        self.bench_exact = bool(bench_exact)
        # -- bench.main, lines 767-805 (world = 1, no collectives) --
        comm = bool(args.force_comm)
        assert not comm, "the harness runs the single-GPU step without collectives"
        if args.chains > 1 and args.defer_da == "window":
            raise SystemExit("--chains > 1 runs with --defer-da off / main / side / layer / bucket")
        tail = args.tail_layers if args.tail_layers >= 0 else 0
        sizes = None
        if args.buckets == 0 and comm and tail == 0:
            sizes = geometric_buckets(args.layers)
        nb = args.buckets if args.buckets > 0 else 8
        torch.manual_seed(0)
        self.wl = wl = bench.build_workload(args, dev, lib, lambda n, ends: FlatGradBucket(
            n, ends, dev, n_buckets=nb, comm_dtype=torch.bfloat16 if args.comm_bf16 else None, force_comm=args.force_comm,
            tail_layers=tail or None, bucket_sizes=sizes), chains=args.chains)
        torch.cuda.synchronize()
        self.opt = opt = None if args.no_optimizer else FlatAdamW(wl["master"], wl["bucket"].flat, wl["work"], lr=1e-4)
        self.cfg = SCH.ScheduleConfig(chains=args.chains, graph=args.graph, topology=args.graph_topology, defer_da=args.defer_da, split_db=bool(args.split_db),
                                      chain_priority=args.chain_priority, fused=bool(args.fused), shadows=args.shadows, shadows_batch=args.shadows_batch == "on",
                                      chain_first=args.capture_order == "chain-first", chain_stagger=args.chain_stagger,
                                      opt_in_backward=args.opt_in_backward == "on", skip=frozenset(skip))
        self.plan = plan = make_plan(wl, args)
        self.inv_keep = float(lib.moka_dropout_scale(float(args.dropout))) if args.dropout > 0 else 1.0
        self.scales: Dict[str, float] = {}
        if not self.bench_exact:
            self._scale_buffers()
        self.sched = SCH.GraphedAdapterStep(wl, self.cfg, args.layers, optimizer=opt, world=1, comm=comm, device=dev)
        before = None if self.bench_exact else self._snapshot()
        self.captured = self.sched.capture() if self.bench_exact else self.sched.capture(restore_grad=True)
        if before is not None:
            # (the capture's warm-up launches are not a step: y / dx as they were; the flat gradient is the executor's to leave as it was)
            for k, t in self._mutable().items():
                t.copy_(before[k[0]][k[1:]])
        torch.cuda.synchronize()
        self.y_pass, self.dx_pass = count_passes(plan.unit_descs())
        self.report: List[Row] = []
        self.epochs: List[int] = []
        self._mask1 = None
        self.k = 0

    # ---------------------------------------------------------------------------------------------------- buffers
    def _sets(self):
        for ci, (sets, _, _, _) in enumerate(self.wl["keep"]):
            for si, (acts, dacts, ys) in enumerate(sets):
                yield ci, si, acts, dacts, ys

    def _mutable(self):
        names = [p[0] for p in _bench().PROJS]
        out = {}
        for ci, si, acts, dacts, ys in self._sets():
            for name, y in zip(names, ys):
                out[("y", ci, si, name)] = y
            for k, t in dacts.items():
                out[("dx", ci, si, k)] = t
        return out

    def _snapshot(self) -> dict:
        snap = {"y": {}, "dx": {}, "acts": {}}
        for k, t in self._mutable().items():
            snap[k[0]][k[1:]] = t.detach().cpu().clone()
        for ci, si, acts, dacts, ys in self._sets():
            for k, t in acts.items():
                snap["acts"][(ci, si, k)] = t.detach().cpu().clone()
        wl, opt = self.wl, self.opt
        snap["work"], snap["master"] = wl["work"].detach().cpu().clone(), wl["master"].detach().cpu().clone()
        if opt is not None:
            snap["m"], snap["v"] = opt.exp_avg.detach().cpu().clone(), opt.exp_avg_sq.detach().cpu().clone()
        return snap

    def _keep(self, epoch: Optional[int]):
        def fn(ci, mb, Tc):
            if self.plan.p <= 0.0:
                return None
            from moka_amd import functional as F
            seed = F.effective_seed(mb.seed, epoch) if epoch is not None else mb.seed
            k = F.dropout_mask(self.plan.p, seed, Tc, mb.d_in, self.dev).cpu()
            return k.double() * self.inv_keep
        return fn

    def _scale_buffers(self):
        """Powers of two that make the adapter term about twice the base it is added to (it then stays within [0.25, 4] of the growing
        base over three steps), from the oracle alone: one oracle step without dropout on zeroed bases gives |term| of every buffer's
        first pass; the dx terms are taken with the scaled y + term as gy."""
        snap = self._snapshot()
        zero = dict(snap, y={k: torch.zeros_like(v) for k, v in snap["y"].items()}, dx={k: torch.zeros_like(v) for k, v in snap["dx"].items()})
        y_t, _, _, _ = oracle_step(self.plan, zero, lambda *a: None)
        mut = self._mutable()

        def pow2(term, base, passes):
            # (|term| of ONE pass: layers that share the set have independent weights, their terms add in quadrature)
            return 2.0 ** round(math.log2(max(term / math.sqrt(passes), 1e-30) / (2.0 * base)))
        y_pass, dx_pass = count_passes(self.plan.unit_descs())
        scaled = dict(zero, y={})
        for k, t in y_t.items():
            s = pow2(t.norm().item(), snap["y"][k].double().norm().item(), y_pass[(k[1], k[2])])
            self.scales["y.chain%d.set%d.%s" % k] = s
            mut[("y",) + k].mul_(s)
            scaled["y"][k] = (snap["y"][k].double() * s).to(torch.bfloat16)
        _, dx_t, _, _ = oracle_step(self.plan, scaled, lambda *a: None)
        for k, t in dx_t.items():
            s = pow2(t.norm().item(), snap["dx"][k].double().norm().item(), dx_pass[(k[1], k[2])])
            self.scales["dx.chain%d.set%d.%s" % k] = s
            mut[("dx",) + k].mul_(s)
        torch.cuda.synchronize()

    # ---------------------------------------------------------------------------------------------------- one step
    def step(self) -> None:
        """One real step, then every check of it (rows appended to self.report)."""
        wl, opt, plan, sched, R = self.wl, self.opt, self.plan, self.sched, self.report
        snap = self._snapshot()
        self.k += 1
        k = self.k
        sched.step(k - 1)
        torch.cuda.synchronize()
        epoch = int(wl["seed_epoch"].item()) if wl.get("seed_epoch") is not None else None
        if epoch is not None:
            self.epochs.append(epoch)
        after = self._snapshot()
        gbuf = wl["gbuf"].detach().cpu().double()
        rows_pre: List[Row] = []
        y_o, dx_o, g_o, peak = oracle_step(plan, snap, self._keep(epoch), y_after=after["y"], rows=None if self.bench_exact else rows_pre, step=k)
        R.extend(rows_pre)

        # ---- y and dx: relative Frobenius error against the oracle's bf16 result, element-wise at most one bf16 ulp per pass (operand-aware
        #      as tests/test_gpu_parity.ulp_bf16_diff: the ulp of the largest value the element held in the snapshot or after any pass)
        for kind, exp, npass in (("y", y_o, self.y_pass), ("dx", dx_o, self.dx_pass)):
            for key, e in exp.items():
                where = "%s.chain%d.set%d.%s" % ((kind,) + key)
                got, e_bf = after[kind][key], e.to(torch.bfloat16)
                R.append(Row(k, kind + ".rel", where, rel(got, e_bf), TOL_BF16))
                R.append(Row(k, kind + ".ulp", where, ulp_bf16_diff(got, e_bf, peak[kind][key]), npass[(key[1], key[2])] + 1e-6))

        # ---- the gradient of every parameter view
        runs_opt = opt is not None and not self.cfg.skips("optimizer")
        if opt is None:
            g_dev = gbuf
        else:
            # the slice zeroes the buffer inside the backward: the gradient it consumed, from the first moment before and after it; what
            # a slice did NOT consume is still in the buffer (and fails the left-zero check below)
            g_dev = recover_grad(after["m"], snap["m"], opt.betas[0], 1.0) + gbuf
        for where, lo, hi, kind in plan.views():
            if opt is not None:
                gn = g_o[lo:hi].norm().item()
                R.append(Row(k, "pre.m_over_g", where, snap["m"][lo:hi].double().norm().item() / gn if gn > 0 else float("inf"), M_OVER_G))
            R.append(Row(k, "grad." + kind, where, rel(g_dev[lo:hi], g_o[lo:hi]), TOL_F32))

        # ---- master against fp64 AdamW on the snapshot and the recovered gradient, bias correction of step k
        if opt is not None:
            p_ref, _, _ = adamw_fp64(snap["master"], snap["m"], snap["v"], g_dev, k, opt.lr, opt.betas, opt.eps, opt.weight_decay)
            for where, lo, hi, kind in plan.views():
                R.append(Row(k, "master", where, rel(after["master"][lo:hi], p_ref[lo:hi]), TOL_ADAMW))

        # ---- bit-exact state
        R.append(Row(k, "state.work", "work == bf16(master)", float((after["work"].view(torch.int16) != after["master"].to(torch.bfloat16).view(torch.int16)).sum()), 0.0))
        if opt is not None:
            R.append(Row(k, "state.grad_left_zero", "gbuf", float((gbuf != 0).sum()) + float(torch.isnan(gbuf).sum()), 0.0))
            R.append(Row(k, "state.t", "opt.t", float(abs(opt.t - k)), 0.0))
            if sched.opt_in_bwd and opt._state is not None:
                R.append(Row(k, "state.t", "device counter", float(abs(int(opt._state[3:4].view(torch.int32).item()) - k)), 0.0))
        r = plan.r
        work = after["work"]
        for ui, (u, up) in enumerate(zip(wl["chains"][0]["units"], plan.chains[0].units)):
            if not up.fused:
                continue
            for m, mb in zip(u.members, up.members):
                Bw = work[mb.off_B:mb.off_B + mb.d_out * r].view(mb.d_out, r)
                bad = float((m["BwT"][:r].cpu().view(torch.int16) != Bw.t().contiguous().view(torch.int16)).sum())
                AT = m["AT"].cpu()
                for mi, o in enumerate(mb.off_A):
                    A = work[o:o + r * mb.d_in].view(r, mb.d_in)
                    bad += float((AT[mi, :, :r].contiguous().view(torch.int16) != A.t().contiguous().view(torch.int16)).sum())
                R.append(Row(k, "state.shadow", "L%d.%s" % (up.layer, mb.name), bad, 0.0))

        # ---- seed epochs: pairwise different words; the same member's keep masks differ from step to step
        if epoch is not None:
            R.append(Row(k, "epoch.distinct", "seed_epoch", float(len(self.epochs) - len(set(self.epochs))), 0.0))
            mb = plan.chains[0].units[0].members[0]
            km = self._keep(epoch)(0, mb, plan.chains[0].B * plan.chains[0].S)
            if self._mask1 is not None:
                R.append(Row(k, "epoch.masks_differ", "chain0.L0.%s" % mb.name, float(torch.equal(km, self._mask1)), 0.0))
            self._mask1 = km

    def run(self, K: int) -> List[Row]:
        for _ in range(K):
            self.step()
        return self.report
