"""Host glue between torch tensors and the C ABI (include/moka_hip.h).

``ops`` are thin 1:1 wrappers of the exported ``moka_X_group`` entry points (pointer extraction,
workspace allocation, current-stream lookup), each with a one-projection form that calls it with
lists of one -- as ``moka_X`` does in the library; ``MokaLinearFn`` is the one autograd node of
1..G adapted projections fed by the same x: frozen base GEMMs on stock PyTorch-ROCm + the MokA
adapters on the HIP kernels, with the explicit backward the reference leaves to autograd
(SURVEY.md section 8, rows a11 and f1).
"""
from __future__ import annotations

import ctypes
from ctypes import POINTER, byref, c_float, c_void_p
from typing import List, Optional, Sequence, Tuple

import torch

from . import _decode_lib, _dlinear_lib, _lib
from .routing import MokaRouting


def _launch_stream(device) -> "torch.cuda.Stream":
    return torch.cuda.current_stream(device)


def _stream_ptr(device) -> c_void_p:
    return c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _require_device(t: torch.Tensor, name: str):
    if not t.is_cuda:
        raise _lib.MokaError(
            f"moka_amd: `{name}` lives on {t.device}; the MokA adapter path only exists as HIP kernels for "
            "MI355X (gfx950) -- there is no CPU fallback (use oracle/ for CPU checking).")


def _storage(tensors, names) -> int:
    """Storage dtype code of one adapted projection: all operands bf16 (the tuned path) or all fp32 (MOKA_F32: exact-fp32 FMA
    kernels, the reference's fp32 configuration -- adapters follow the base dtype, layer.py:124-132)."""
    dts = {t.dtype for t in tensors}
    if dts == {torch.bfloat16}:
        return _lib.MOKA_BF16
    if dts == {torch.float32}:
        return _lib.MOKA_F32
    desc = ", ".join(f"{n}: {t.dtype}" for n, t in zip(names, tensors))
    raise _lib.MokaError(f"moka_amd: operands must be all bf16 or all fp32 on the HIP path ({desc})")


def _dense(t: torch.Tensor) -> torch.Tensor:
    """`t` as the kernels take an operand: contiguous AND on a 16-byte boundary (include/moka_hip.h, pointer alignment) -- a copy where it
    is not.  A contiguous view at an odd element offset of a packed buffer is as unusable as a strided one: the library refuses it."""
    if t.is_contiguous():
        return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)
    return t.contiguous()


def _ptrs(tensors: Sequence[torch.Tensor]):
    return (c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _floats(vals: Sequence[float]):
    return (c_float * len(vals))(*[float(v) for v in vals])


# --------------------------------------------------------------------------------------
# 1:1 wrappers of the C entry points: G projections fed by the same x (q/k/v, gate/up), G >= 1
# --------------------------------------------------------------------------------------
def _ints(vals: Sequence[int]):
    return (ctypes.c_int * len(vals))(*[int(v) for v in vals])


def _u64s(vals: Sequence[int]):
    return (ctypes.c_ulonglong * len(vals))(*[int(v) for v in vals])


def _optptrs(tensors: Optional[Sequence[Optional[torch.Tensor]]]):
    """A pointer array with NULL for the members that are None; NULL for no array at all."""
    if tensors is None:
        return None
    return (c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


class FwdState:
    """Rank-space results of the forward that the up-projection and the backward consume."""
    __slots__ = ("h", "hp", "hp_tok", "hp_kmj", "BwT", "AT")


def _fwd_state(T: int, RP: int, dev, want_hp: bool = False, want_tok: bool = False, Bw: Optional[torch.Tensor] = None,
               A: Optional[Sequence[torch.Tensor]] = None) -> FwdState:
    """The buffers one projection's forward writes: h and hp_kmj always; hp / hp_tok on request; the shadows of the weights given."""
    Tp = _lib.tok_pad(T)
    st = FwdState()
    st.h = torch.empty((T, RP), dtype=torch.float32, device=dev)
    st.hp = torch.empty((T, RP), dtype=torch.float32, device=dev) if want_hp else None
    st.hp_tok = torch.empty((Tp, 2 * RP), dtype=torch.bfloat16, device=dev) if want_tok else None
    st.hp_kmj = torch.empty((2, RP, Tp), dtype=torch.bfloat16, device=dev)
    st.BwT = torch.empty((RP, Bw.shape[0]), dtype=torch.bfloat16, device=dev) if Bw is not None else None
    st.AT = torch.empty((len(A), A[0].shape[1], RP), dtype=torch.bfloat16, device=dev) if A is not None else None
    return st


class BwdState:
    __slots__ = ("dh", "dh_tok", "dh_kmj")


def _bwd_state(T: int, RP: int, M: int, dev, want_dh: bool = False) -> BwdState:
    Tp = _lib.tok_pad(T)
    st = BwdState()
    st.dh = torch.empty((T, RP), dtype=torch.float32, device=dev) if want_dh else None
    st.dh_tok = torch.empty((Tp, 2 * RP), dtype=torch.bfloat16, device=dev)
    st.dh_kmj = torch.empty((M, 2, RP, Tp), dtype=torch.bfloat16, device=dev)
    return st


def down_fwd_group(x2: torch.Tensor, A: Sequence[Sequence[torch.Tensor]], rt: MokaRouting, r: int, s_in: float,
                   dropout_p: float = 0.0, seeds: Optional[Sequence[int]] = None, seed_dev: Optional[torch.Tensor] = None,
                   dtype: int = _lib.MOKA_BF16) -> List[torch.Tensor]:
    """One read of x2 [T,d_in] for the G down-projections A[g][m]; returns the G split-K partial buffers
    part [ks,T,RP] fp32 (the slices of s_in * drop(x) A_mod^T)."""
    lib = _lib.load()
    T, d_in = x2.shape
    G, M = len(A), len(A[0])
    RP = _lib.rank_pad(r)
    ks = _lib.ksplit(T, d_in, r, G)
    parts = [torch.empty((ks, T, RP), dtype=torch.float32, device=x2.device) for _ in range(G)]
    _lib.check(lib.moka_down_fwd_group(x2.data_ptr(), _ptrs([a for Ag in A for a in Ag]), rt.tok_mod.data_ptr(), _ptrs(parts),
                                       T, d_in, r, M, G, float(s_in), float(dropout_p),
                                       _u64s(seeds if seeds is not None else [0] * G), dtype,
                                       _det_opts(x2.device, T, d_in, r, G, M, seed_dev, want_det=False), _stream_ptr(x2.device)), "moka_down_fwd_group")
    return parts


def cross_fwd_group(parts: Sequence[torch.Tensor], rt: MokaRouting, r: int, s_out: Sequence[float], w: float, inv_sqrt_dk: float,
                    Bw: Optional[Sequence[torch.Tensor]] = None, A: Optional[Sequence[Sequence[torch.Tensor]]] = None,
                    want_tok: bool = True, want_hp: bool = False) -> List[FwdState]:
    """Bw / A: the weights whose shadows (BwT / AT) the launch writes as well; None: neither allocated nor requested.
    want_tok=False: the token-major pack is not written (the up-projection is `up_fwd_fused_group_`, which computes it itself)."""
    lib = _lib.load()
    G = len(parts)
    ks, T, RP = parts[0].shape
    dev = parts[0].device
    sts = [_fwd_state(T, RP, dev, want_hp, want_tok, None if Bw is None else Bw[g], None if A is None else A[g]) for g in range(G)]
    _lib.check(lib.moka_cross_fwd_group(_ptrs(parts), ks, byref(rt.struct), _floats(s_out),
                                        _optptrs(Bw), None if Bw is None else _ints([b.shape[0] for b in Bw]),
                                        None if A is None else _ptrs([a for Ag in A for a in Ag]), 0 if A is None else A[0][0].shape[1],
                                        _ptrs([st.h for st in sts]), _ptrs([st.hp for st in sts]) if want_hp else None,
                                        _ptrs([st.hp_tok for st in sts]) if want_tok else None, _ptrs([st.hp_kmj for st in sts]),
                                        None if Bw is None else _ptrs([st.BwT for st in sts]),
                                        None if A is None else _ptrs([st.AT for st in sts]),
                                        G, r, float(w), float(inv_sqrt_dk), _stream_ptr(dev)), "moka_cross_fwd_group")
    return sts


def up_fwd_group_(ys: Sequence[torch.Tensor], hp_toks: Sequence[torch.Tensor], Bw: Sequence[torch.Tensor], rt: MokaRouting, r: int,
                  dtype: int = _lib.MOKA_BF16):
    """In place: ys[g] [T,d_out_g] += (s_out[mod] hp_g) Bw_g^T (the scale is already inside hp_toks[g])."""
    lib = _lib.load()
    T = ys[0].shape[0]
    _lib.check(lib.moka_up_fwd_group(_ptrs(hp_toks), _ptrs(Bw), rt.tok_mod.data_ptr(), _ptrs(ys), T, r,
                                     _ints([y.shape[1] for y in ys]), len(ys), dtype, _stream_ptr(ys[0].device)),
               "moka_up_fwd_group")


def up_fwd_fused_group_(ys: Sequence[torch.Tensor], parts: Sequence[torch.Tensor], Bw: Sequence[torch.Tensor], rt: MokaRouting, r: int,
                        s_out: Sequence[float], w: float, inv_sqrt_dk: float, want_state: bool = False) -> Optional[List[FwdState]]:
    """In place: ys[g] [T,d_out] bf16 += (s_out[mod] hp_g) Bw_g^T with hp_g computed from the split-K slices `parts[g]` inside the kernel
    (the bits of cross_fwd_group + up_fwd_group_; bf16 storage).  want_state: the launch also writes what the backward reads from
    the rank space (h, hp_kmj); returned as FwdStates whose BwT / AT are filled by `weight_shadows_group`."""
    lib = _lib.load()
    ks, T, RP = parts[0].shape
    sts = [_fwd_state(T, RP, parts[0].device) for _ in ys] if want_state else None
    _lib.check(lib.moka_up_fwd_fused_group(_ptrs(parts), ks, byref(rt.struct), _floats(s_out), _ptrs(Bw), _ptrs(ys),
                                           _ints([y.shape[1] for y in ys]),
                                           None if sts is None else _ptrs([st.h for st in sts]),
                                           None if sts is None else _ptrs([st.hp_kmj for st in sts]),
                                           len(ys), r, float(w), float(inv_sqrt_dk),
                                           _lib.MOKA_BF16, _stream_ptr(ys[0].device)), "moka_up_fwd_fused_group")
    return sts


def weight_shadows_group(Bws: Optional[Sequence[torch.Tensor]], As: Optional[Sequence[Sequence[torch.Tensor]]], r: int):
    """Per projection (BwT [RP, d_out], AT [M, d_in, RP]) bf16 in one launch: the transposed, zero-padded weight copies the backward kernels
    read -- functions of the weights alone (moka_weight_shadows), so they need not sit on the forward's dependency chain.  BwT only when
    `Bws` is given, AT only when `As` is."""
    lib = _lib.load()
    RP = _lib.rank_pad(r)
    dev = Bws[0].device if Bws is not None else As[0][0].device
    BwTs = [torch.empty((RP, b.shape[0]), dtype=torch.bfloat16, device=dev) for b in Bws] if Bws is not None else None
    ATs = [torch.empty((len(Ag), Ag[0].shape[1], RP), dtype=torch.bfloat16, device=dev) for Ag in As] if As is not None else None
    _lib.check(lib.moka_weight_shadows_group(_optptrs(Bws), None if Bws is None else _ints([b.shape[0] for b in Bws]),
                                             None if As is None else _ptrs([a for Ag in As for a in Ag]), 0 if As is None else As[0][0].shape[1],
                                             _optptrs(BwTs), _optptrs(ATs),
                                             len(Bws if Bws is not None else As), r, len(As[0]) if As is not None else 1, _stream_ptr(dev)),
               "moka_weight_shadows_group")
    return BwTs, ATs


def weight_shadows_batch_(Bws: Sequence[torch.Tensor], As: Sequence[Sequence[torch.Tensor]], r: int,
                          BwTs: Sequence[torch.Tensor], ATs: Sequence[torch.Tensor]) -> None:
    """Rewrite the shadows (BwT [RP, d_out], AT [M, d_in, RP]) of n projections of ANY widths in place, one launch per MOKA_MAX_SHADOW_BATCH
    of them: what a trainer that keeps persistent shadows runs behind an optimizer step (moka_weight_shadows_batch)."""
    lib = _lib.load()
    M = len(As[0])
    for i in range(0, len(Bws), _lib.MOKA_MAX_SHADOW_BATCH):
        j = min(len(Bws), i + _lib.MOKA_MAX_SHADOW_BATCH)
        _lib.check(lib.moka_weight_shadows_batch(_ptrs(Bws[i:j]), _ints([b.shape[0] for b in Bws[i:j]]), _ptrs([a for Ag in As[i:j] for a in Ag]),
                                                 _ints([Ag[0].shape[1] for Ag in As[i:j]]), _ptrs(BwTs[i:j]), _ptrs(ATs[i:j]), j - i, r, M,
                                                 _stream_ptr(Bws[0].device)), "moka_weight_shadows_batch")


def up_bwd_group(gys: Sequence[torch.Tensor], hp_kmjs: Optional[Sequence[torch.Tensor]], BwTs: Optional[Sequence[torch.Tensor]],
                 rt: MokaRouting, r: int, s_out: Sequence[float], dB_accs: Optional[Sequence[torch.Tensor]], want_g: bool = True,
                 dtype: int = _lib.MOKA_BF16) -> Optional[List[torch.Tensor]]:
    """gys[g] [T,d_out_g] -> g_parts[g] [ks,T,RP] (want_g=False: skip); dB_accs[g] [d_out_g,r] fp32 += (may be None: skip)."""
    lib = _lib.load()
    G = len(gys)
    T = gys[0].shape[0]
    RP = _lib.rank_pad(r)
    d_outs = [g_.shape[1] for g_ in gys]
    ks = _lib.ksplit_bwd(T, max(d_outs), r)
    g_parts = [torch.empty((ks, T, RP), dtype=torch.float32, device=gys[0].device) for _ in range(G)] if want_g else None
    _lib.check(lib.moka_up_bwd_group(_ptrs(gys), _optptrs(hp_kmjs), _optptrs(BwTs), rt.tok_mod.data_ptr(), _floats(s_out),
                                     _optptrs(g_parts), _optptrs(dB_accs),
                                     T, r, _ints(d_outs), len(s_out), G, dtype,
                                     _det_opts(gys[0].device, T, max(d_outs), r, G, len(s_out)) if dB_accs is not None else None,
                                     _stream_ptr(gys[0].device)),
               "moka_up_bwd_group")
    return g_parts


def cross_bwd_group(g_parts: Sequence[torch.Tensor], hs: Sequence[torch.Tensor], rt: MokaRouting, r: int, s_in: float,
                    w: float, inv_sqrt_dk: float, want_dh: bool = False) -> List[BwdState]:
    lib = _lib.load()
    G = len(g_parts)
    ks, T, RP = g_parts[0].shape
    dev = g_parts[0].device
    sts = [_bwd_state(T, RP, rt.M, dev, want_dh) for _ in range(G)]
    _lib.check(lib.moka_cross_bwd_group(_ptrs(g_parts), ks, _ptrs(hs), byref(rt.struct), float(s_in),
                                        _ptrs([st.dh for st in sts]) if want_dh else None,
                                        _ptrs([st.dh_tok for st in sts]), _ptrs([st.dh_kmj for st in sts]),
                                        _ptrs([rt.cross_ws(r, g) for g in range(G)]), G, r, float(w), float(inv_sqrt_dk),
                                        _stream_ptr(dev)), "moka_cross_bwd_group")
    return sts


def down_bwd_group_(bsts: Sequence[BwdState], x2: torch.Tensor, ATs: Optional[Sequence[torch.Tensor]], rt: MokaRouting, r: int,
                    dA_accs: Optional[Sequence[Sequence[torch.Tensor]]], dx2: Optional[torch.Tensor],
                    dropout_p: float = 0.0, seeds: Optional[Sequence[int]] = None, seed_dev: Optional[torch.Tensor] = None,
                    dtype: int = _lib.MOKA_BF16):
    """dA_accs[g][m] [r,d_in] fp32 += (one read of x2 for all G); dx2 [T,d_in] += sum_g dh_g A_g (one read-modify-write); either may be None."""
    lib = _lib.load()
    T, d_in = x2.shape
    G = len(bsts)
    _lib.check(lib.moka_down_bwd_group(_ptrs([b.dh_tok for b in bsts]), _optptrs([b.dh_kmj for b in bsts]), x2.data_ptr(),
                                       _optptrs(ATs), rt.tok_mod.data_ptr(),
                                       None if dA_accs is None else _ptrs([a for Ag in dA_accs for a in Ag]),
                                       None if dx2 is None else dx2.data_ptr(), T, d_in, r, rt.M, G, float(dropout_p),
                                       _u64s(seeds if seeds is not None else [0] * G), dtype,
                                       _det_opts(x2.device, T, d_in, r, G, rt.M, seed_dev, want_det=dA_accs is not None), _stream_ptr(x2.device)),
               "moka_down_bwd_group")


# --------------------------------------------------------------------------------------
# one projection: the same entry points as a group of one (as moka_X is moka_X_group(G = 1) in the library)
# --------------------------------------------------------------------------------------
def _one(t):
    return None if t is None else [t]


def down_fwd(x2: torch.Tensor, A: Sequence[torch.Tensor], rt: MokaRouting, r: int, s_in: float,
             dropout_p: float = 0.0, seed: int = 0, dtype: int = 0, seed_dev: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x2 [T,d_in] bf16 -> part [ks,T,RP] fp32 (split-K partials of s_in * drop(x) A_mod^T)."""
    return down_fwd_group(x2, [A], rt, r, s_in, dropout_p, [seed], seed_dev, dtype)[0]


def cross_fwd(part: torch.Tensor, rt: MokaRouting, r: int, s_out: Sequence[float], w: float, inv_sqrt_dk: float,
              Bw: Optional[torch.Tensor] = None, want_hp: bool = False, A: Optional[Sequence[torch.Tensor]] = None,
              want_tok: bool = True) -> FwdState:
    return cross_fwd_group([part], rt, r, s_out, w, inv_sqrt_dk, _one(Bw), _one(A), want_tok, want_hp)[0]


def up_fwd_fused_(y2: torch.Tensor, part: torch.Tensor, Bw: torch.Tensor, rt: MokaRouting, r: int, s_out: Sequence[float],
                  w: float, inv_sqrt_dk: float, want_state: bool = False) -> Optional[FwdState]:
    sts = up_fwd_fused_group_([y2], [part], [Bw], rt, r, s_out, w, inv_sqrt_dk, want_state)
    return None if sts is None else sts[0]


def weight_shadows(Bw: Optional[torch.Tensor], A: Optional[Sequence[torch.Tensor]], r: int) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    BwTs, ATs = weight_shadows_group(_one(Bw), _one(A), r)
    return None if BwTs is None else BwTs[0], None if ATs is None else ATs[0]


def up_fwd_(y2: torch.Tensor, hp_tok: torch.Tensor, Bw: torch.Tensor, rt: MokaRouting, r: int, dtype: int = 0):
    up_fwd_group_([y2], [hp_tok], [Bw], rt, r, dtype)
    return y2


def up_bwd(gy2: torch.Tensor, hp_kmj: Optional[torch.Tensor], BwT: Optional[torch.Tensor], rt: MokaRouting, r: int,
           s_out: Sequence[float], dB_acc: Optional[torch.Tensor], dtype: int = 0, want_g: bool = True) -> Optional[torch.Tensor]:
    g_parts = up_bwd_group([gy2], _one(hp_kmj), _one(BwT), rt, r, s_out, _one(dB_acc), want_g, dtype)
    return None if g_parts is None else g_parts[0]


def cross_bwd(g_part: torch.Tensor, h: torch.Tensor, rt: MokaRouting, r: int, s_in: float, w: float, inv_sqrt_dk: float,
              want_dh: bool = False) -> BwdState:
    return cross_bwd_group([g_part], [h], rt, r, s_in, w, inv_sqrt_dk, want_dh)[0]


def down_bwd_(bst: BwdState, x2: torch.Tensor, AT: Optional[torch.Tensor], rt: MokaRouting, r: int,
              dA_acc: Optional[Sequence[torch.Tensor]], dx2: Optional[torch.Tensor],
              dropout_p: float = 0.0, seed: int = 0, dtype: int = 0, seed_dev: Optional[torch.Tensor] = None):
    down_bwd_group_([bst], x2, _one(AT), rt, r, _one(dA_acc), dx2, dropout_p, [seed], seed_dev, dtype)


def down_bwd_da_batch_(dh_kmjs: Sequence[torch.Tensor], xs: Sequence[torch.Tensor], rt: MokaRouting, r: int,
                       dA_accs: Sequence[Sequence[torch.Tensor]], dropout_p: float = 0.0, seeds: Optional[Sequence[int]] = None,
                       seed_dev: Optional[torch.Tensor] = None):
    """dA_accs[i][m] += for n independent projections of one token set (their own x [T, d_in_i] and operand pack) in ONE launch: what a
    trainer defers per decoder layer (moka_down_bwd_da_batch; with the deterministic mode on: one launch per projection)."""
    lib = _lib.load()
    n, T = len(xs), xs[0].shape[0]
    d_ins = [int(x.shape[1]) for x in xs]
    _lib.check(lib.moka_down_bwd_da_batch(_ptrs(dh_kmjs), _ptrs(xs), (ctypes.c_int * n)(*d_ins), rt.tok_mod.data_ptr(),
                                          _ptrs([a for Ai in dA_accs for a in Ai]), n, T, r, rt.M, float(dropout_p),
                                          _u64s(seeds if seeds is not None else [0] * n), _lib.MOKA_BF16,
                                          _det_opts(xs[0].device, T, max(d_ins), r, 1, rt.M, seed_dev), _stream_ptr(xs[0].device)),
               "moka_down_bwd_da_batch")


def up_bwd_db_batch_(gys: Sequence[torch.Tensor], hp_kmjs: Sequence[torch.Tensor], rt: MokaRouting, r: int, dB_accs: Sequence[torch.Tensor]):
    """dB_accs[i] [d_out_i, r] += for n independent projections of one token set in ONE launch (moka_up_bwd_db_batch): the deferred dB of a
    decoder layer at the ranks where dB is a pass of its own."""
    lib = _lib.load()
    n, T = len(gys), gys[0].shape[0]
    d_outs = [int(g.shape[1]) for g in gys]
    _lib.check(lib.moka_up_bwd_db_batch(_ptrs(gys), _ptrs(hp_kmjs), (ctypes.c_int * n)(*d_outs), rt.tok_mod.data_ptr(), _ptrs(dB_accs), n, T, r, rt.M,
                                        _lib.MOKA_BF16, _det_opts(gys[0].device, T, max(d_outs), r, 1, rt.M), _stream_ptr(gys[0].device)),
               "moka_up_bwd_db_batch")


def dropout_mask(dropout_p: float, seed: int, T: int, d_in: int, device) -> torch.Tensor:
    """The keep mask (uint8 [T,d_in]) the kernels derive from (dropout_p, seed) -- for checkers."""
    lib = _lib.load()
    out = torch.empty((T, d_in), dtype=torch.uint8, device=device)
    _lib.check(lib.moka_dropout_mask(float(dropout_p), int(seed), T, d_in, out.data_ptr(), _stream_ptr(device)), "moka_dropout_mask")
    return out


def _token_scale(rt: MokaRouting, s_out: Sequence[float], device) -> torch.Tensor:
    """s_out[mod(t)] per token (0 for tokens of no modality), fp32 [T] -- the scale the bf16 packs carry built in."""
    lut = torch.zeros(256, dtype=torch.float32, device=device)
    lut[:len(s_out)] = torch.tensor([float(v) for v in s_out], dtype=torch.float32, device=device)
    return lut[rt.tok_mod[:rt.T].long()]


# Deterministic mode is HOST-side state of this Python module: the library itself keeps none (the workspace travels with every
# backward call as `moka_opts`).  One workspace per (device, stream): calls that run concurrently on two streams never share one.
_DET_ON = {}            # device -> True
_DET_WS = {}            # (device, stream handle) -> uint8 workspace tensor


def set_deterministic(enabled: bool, T: int = 0, C_max: int = 0, r: int = 16, G: int = 3, M: int = 3, device=None) -> None:
    """Bitwise-reproducible weight gradients: the dA_m / dB kernels write one partial tile per token run into a workspace and a
    second launch adds the runs in order, instead of fp32 atomics.  The setting is per device and lives here, not in the library;
    the workspace of a call is sized for THAT call (``moka_deterministic_ws_bytes``), allocated on first use per stream, kept
    alive and handed to the backward entry points through ``moka_opts``.  The size arguments are optional pre-allocation hints
    for the current stream."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    if not enabled:
        _DET_ON.pop(dev, None)
        for k in [k for k in _DET_WS if k[0] == dev]:
            del _DET_WS[k]
        return
    _DET_ON[dev] = True
    if T and C_max:
        if _det_opts(dev, int(T), int(C_max), int(r), int(G), int(M)) is None:
            raise ValueError("set_deterministic: bad T / C_max / r / G / M")


def _det_opts(device, T: int, C_max: int, r: int, G: int, M: int, seed_dev: Optional[torch.Tensor] = None, want_det: bool = True):
    """moka_opts of one call: the deterministic-mode workspace (set_deterministic on for the device and the call produces weight gradients)
    and / or the device-resident part of the dropout seed (``seed_dev``: an int64 tensor of one element); None when neither applies."""
    sd = None if seed_dev is None else seed_dev.data_ptr()
    dev = torch.device(device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    if not want_det or not _DET_ON.get(dev):
        return None if sd is None else ctypes.byref(_lib.MokaOpts(seed_dev=sd))
    n = int(_lib.load().moka_deterministic_ws_bytes(int(T), int(C_max), int(r), int(G), int(M)))
    if n == 0:
        return None if sd is None else ctypes.byref(_lib.MokaOpts(seed_dev=sd))
    key = (dev, _launch_stream(dev).cuda_stream)
    ws = _DET_WS.get(key)
    if ws is None or ws.numel() < n:
        ws = torch.empty(n, dtype=torch.uint8, device=dev)
        _DET_WS[key] = ws
    return ctypes.byref(_lib.MokaOpts(ws.data_ptr(), ws.numel(), seed_dev=sd))


def effective_seed(seed: int, epoch: int) -> int:
    """The seed whose mask a call with (seed, *seed_dev == epoch) uses: 32-bit halves, low ^ low and high + high (include/moka_hip.h,
    moka_opts.seed_dev) -- what a checker hands to ``dropout_mask`` to replay a captured step's masks."""
    seed, epoch = int(seed) & (2 ** 64 - 1), int(epoch) & (2 ** 64 - 1)
    lo = (seed ^ epoch) & 0xffffffff
    hi = ((seed >> 32) + (epoch >> 32)) & 0xffffffff
    return (hi << 32) | lo


def draw_seed() -> int:
    """Per-call dropout seed from torch's CPU generator (torch.manual_seed controls it; activation
    checkpointing restores that generator before the re-forward, so the mask replays)."""
    a, b = torch.randint(0, 2 ** 31 - 1, (2,)).tolist()
    return (a << 31) | b


def _grad_accumulators(shapes: Sequence[Tuple[int, int]], device) -> Tuple[torch.Tensor, List[torch.Tensor]]:
    """One zeroed fp32 buffer carved into the [rows, cols] accumulators the weight-gradient kernels add into
    (one memset and, afterwards, one cast for all of them instead of one tiny kernel per tensor)."""
    sizes = [a * b for a, b in shapes]
    flat = torch.zeros(sum(sizes), dtype=torch.float32, device=device)
    views, off = [], 0
    for (a, b), n in zip(shapes, sizes):
        views.append(flat[off:off + n].view(a, b))
        off += n
    return flat, views


def _check_sinks(dB_acc, dA_acc, d_out: int, r: int, d_in: int, M: int, device) -> None:
    ts = ([dB_acc] if dB_acc is not None else []) + (list(dA_acc) if dA_acc is not None else [])
    if dA_acc is not None and len(dA_acc) != M:
        raise ValueError(f"moka_amd: {len(dA_acc)} gradient sinks for {M} lora_A matrices")
    for t in ts:
        if t.dtype != torch.float32 or not t.is_contiguous() or t.device != device:
            raise TypeError("moka_amd: gradient sinks must be contiguous fp32 tensors on the device of the activations")
    if dB_acc is not None and tuple(dB_acc.shape) != (d_out, r):
        raise ValueError(f"moka_amd: lora_B gradient sink is {tuple(dB_acc.shape)}, expected {(d_out, r)}")
    if dA_acc is not None:
        for t in dA_acc:
            if tuple(t.shape) != (r, d_in):
                raise ValueError(f"moka_amd: lora_A gradient sink is {tuple(t.shape)}, expected {(r, d_in)}")


def _split_like(flat: torch.Tensor, shapes: Sequence[Tuple[int, int]]) -> List[torch.Tensor]:
    out, off = [], 0
    for a, b in shapes:
        out.append(flat[off:off + a * b].view(a, b))
        off += a * b
    return out


# The forward of the autograd node: True (default) = moka_down_fwd -> moka_up_fwd_fused (+ moka_weight_shadows) where the fused launch
# exists (bf16 storage) and pays for the shape (moka_up_fwd_fused_pays: not at rank pad 64); False = the three-launch path moka_down_fwd -> moka_cross_fwd -> moka_up_fwd.  Same bits either way
# (tests/test_gpu_fused.py); a module-level switch for A/B runs, not a tuning knob.
FUSE_FORWARD = True

# Cached decode steps (masks None, no autograd, a handful of tokens): True = the base GEMMs + ONE moka_decode_fwd launch per
# projection group (include/moka_decode.h: no split-K slices, no backward state, no weight shadows); False (default) = the autograd node
# below, as for training.  A module-level switch for A/B runs (tools/decode_step.py), not a tuning knob.  It ships OFF: the kernel is
# tested for correctness, but no timing of it against the general path is recorded yet ("Cached decode steps"); the
# default turns on with that record.
DECODE_FORWARD = False
decode_launches = 0      # moka_decode_fwd calls made by moka_linear / moka_linear_group so far (tests and tools/decode_step.py read it)


def _step_call(switch_on: bool, is_plain: bool, dtype: int, dropout_ps: Sequence[float], grad_recorded: bool) -> bool:
    """What both decode-step libraries ask of a call before they look at its shape: their switch is on, the routing is
    ``MokaRouting.plain``, bf16 storage, no dropout, autograd records nothing."""
    return bool(switch_on and is_plain) and dtype == _lib.MOKA_BF16 and not grad_recorded and not any(p > 0.0 for p in dropout_ps)


def decode_serves(switch_on: bool, is_plain: bool, dtype: int, dropout_ps: Sequence[float], grad_recorded: bool,
                  T: int, d_in: int, d_outs: Sequence[int], r: int) -> bool:
    """Does the decode-step kernel take this call?  Plain values in, so the rule can be checked without a device: ``_step_call``, and
    the library accepts the shape (moka_decode_ok: at most moka_decode_max_tokens tokens, at most three projections)."""
    if not _step_call(switch_on, is_plain, dtype, dropout_ps, grad_recorded):
        return False
    return _decode_lib.decode_ok(T, d_in, d_outs, r, dtype)


# Cached decode steps of at most moka_dlinear_max_tokens (16) tokens: True = ONE moka_dlinear_fwd launch per projection group computes the
# base GEMV, the bias and the adapter term (include/moka_dlinear.h: W is streamed once, y is rounded once, no torch.nn.functional.linear
# call); False (default) = the paths below it, as DECODE_FORWARD says.  It is asked BEFORE DECODE_FORWARD and does not depend on it.  A
# module-level switch for A/B runs (tools/decode_step.py, mode `fused`), not a tuning knob; it ships OFF and turns on, if at all, from
# the record in DESIGN.md section 6.
DLINEAR_FORWARD = False
dlinear_launches = 0     # moka_dlinear_fwd calls made by moka_linear / moka_linear_group so far (tests and tools/decode_step.py read it)


def dlinear_serves(switch_on: bool, is_plain: bool, dtype: int, dropout_ps: Sequence[float], grad_recorded: bool,
                   T: int, d_in: int, d_outs: Sequence[int], r: int, weights_row_major: bool, biases_ok: bool) -> bool:
    """Does the fused decode-step projection take this call?  Plain values in, as for ``decode_serves``: ``_step_call``, every base
    weight is a contiguous row-major [d_out, d_in] matrix (not the transposed view of a ``fan_in_fan_out`` layer), every bias is absent
    or contiguous bf16, and the library accepts the shape (moka_dlinear_ok: at most moka_dlinear_max_tokens tokens, at most three
    projections)."""
    if not (_step_call(switch_on, is_plain, dtype, dropout_ps, grad_recorded) and weights_row_major and biases_ok):
        return False
    return _dlinear_lib.dlinear_ok(T, d_in, d_outs, r, dtype)


def _decode_forward(x, projections, rt: MokaRouting, specs):
    """The outputs of a plain-routing call on the decode-step kernel, or None when the call belongs to the autograd node (which also
    raise the errors of a malformed call).  Gathers the plain values of the call once, asks ``dlinear_serves`` where its switch is on, then
    ``decode_serves``, and gathers the operands once for whichever library takes the call.

    "Autograd records nothing" is judged per call, so a no-grad pass over TRAINABLE adapters is a decode call as well: under reentrant
    activation checkpointing the first forward of a masks-None call of at most moka_decode_max_tokens tokens takes this kernel and the
    recompute takes the autograd node.  The two outputs agree to the last bits of bf16 (tests/test_gpu_decode.py: both are within one ulp
    of the oracle), the gradients are those of the node; set DECODE_FORWARD = False where bit-equal recomputation matters."""
    sp = specs[0]
    tensors = []
    for (W, b, Bw, A), o in zip(projections, specs):
        if W is None or len(A) != rt.M or len(o.s_out) != rt.M:          # adapter term alone / a malformed call: not one fused call
            return None
        if (o.r, o.s_in, o.s_out) != (sp.r, sp.s_in, sp.s_out):          # one rank and one scale per launch
            return None
        tensors += [W, Bw, *A] + ([b] if b is not None else [])
    d_in = x.shape[-1]
    T = x.numel() // d_in
    kinds = {t.dtype for t in tensors} | {x.dtype}
    dtype = {torch.bfloat16: _lib.MOKA_BF16, torch.float32: _lib.MOKA_F32}.get(next(iter(kinds))) if len(kinds) == 1 else None
    if dtype is None or not x.is_cuda or T != rt.T:
        return None
    recorded = torch.is_grad_enabled() and (x.requires_grad or any(t.requires_grad for t in tensors))
    d_outs = [int(Bw.shape[0]) for (_, _, Bw, _) in projections]
    dropout_ps = [o.dropout_p for o in specs]
    fused = False
    if DLINEAR_FORWARD:                                                      # (off: none of the layout checks is evaluated, the call is today's)
        row_major = all(W.dim() == 2 and tuple(W.shape) == (d, d_in) and W.is_contiguous() and W.data_ptr() % 16 == 0
                        for (W, _, _, _), d in zip(projections, d_outs))
        biases_ok = all(b is None or (b.dtype == torch.bfloat16 and b.dim() == 1 and b.is_contiguous() and b.data_ptr() % 16 == 0)
                        for (_, b, _, _) in projections)
        fused = dlinear_serves(True, rt.is_plain, dtype, dropout_ps, recorded, T, d_in, d_outs, sp.r, row_major, biases_ok)
    if not fused and not decode_serves(DECODE_FORWARD, rt.is_plain, dtype, dropout_ps, recorded, T, d_in, d_outs, sp.r):
        return None
    global decode_launches, dlinear_launches
    x2 = _dense(x.reshape(-1, d_in))
    As = [_dense(A[0]) for (_, _, _, A) in projections]                                        # masks None: the text adapter alone
    Bws = [_dense(Bw) for (_, _, Bw, _) in projections]
    scale, stream = float(sp.s_in * sp.s_out[0]), _stream_ptr(x2.device)
    if fused:
        ys = [torch.empty(T, d, dtype=x2.dtype, device=x2.device) for d in d_outs]             # written, never read
        bs = [b for (_, b, _, _) in projections]
        bias_arr = None if all(b is None for b in bs) else (c_void_p * len(bs))(*[None if b is None else b.data_ptr() for b in bs])
        _dlinear_lib.check(_dlinear_lib.load().moka_dlinear_fwd(
            x2.data_ptr(), _ptrs([W for (W, _, _, _) in projections]), bias_arr, _ptrs(As), _ptrs(Bws), _ptrs(ys), _ints(d_outs),
            len(ys), T, d_in, sp.r, scale, stream), "moka_dlinear_fwd")
        dlinear_launches += 1
    else:
        ys = [_dense(torch.nn.functional.linear(x2, W, b)) for (W, b, _, _) in projections]    # frozen base, stock PyTorch-ROCm
        _decode_lib.check(_decode_lib.load().moka_decode_fwd(x2.data_ptr(), _ptrs(As), _ptrs(Bws), _ptrs(ys), _ints(d_outs), len(ys), T, d_in,
                                                             sp.r, scale, stream), "moka_decode_fwd")
        decode_launches += 1
    return [y.reshape(*x.shape[:-1], y.shape[-1]) for y in ys]


# --------------------------------------------------------------------------------------
# autograd node of 1..G adapted projections fed by the same x
# --------------------------------------------------------------------------------------
class AdapterSpec:
    """Static description of one adapted projection (what varies between AVT and VT)."""

    __slots__ = ("r", "s_in", "s_out", "w", "inv_sqrt_dk", "dropout_p", "seed", "sinks", "defer", "shadows", "seed_dev")

    def __init__(self, r: int, s_in: float, s_out: Sequence[float], w: float, inv_sqrt_dk: float,
                 dropout_p: float = 0.0, seed: Optional[int] = None, sinks=None, defer=None, shadows=None, seed_dev=None):
        self.r, self.s_in, self.s_out, self.w, self.inv_sqrt_dk = int(r), float(s_in), [float(s) for s in s_out], float(w), float(inv_sqrt_dk)
        self.dropout_p = float(dropout_p)
        self.seed = (draw_seed() if seed is None else int(seed)) if self.dropout_p > 0.0 else 0
        # sinks = (dB_acc [d_out, r] fp32, [dA_acc_m [r, d_in] fp32 ...]): views of a flat gradient buffer
        # (moka_amd.parallel.attach) the weight-gradient kernels accumulate into DIRECTLY; the autograd node then returns no
        # gradient for lora_B / lora_A (the data-parallel step works on the flat buffer).  None: ordinary autograd gradients.
        self.sinks = sinks
        # defer: callable(fn) installed with the sinks (moka_amd.parallel.attach(defer_dA=True)).  dA_m is needed by the optimizer
        # only: the backward then runs the dx half of moka_down_bwd on the dependency chain and hands the dA_m half to `defer`,
        # which launches it later on a side stream (beside the next layer's chain), before the gradients are used.
        self.defer = defer
        # shadows = (BwT [RP, d_out], AT [M, d_in, RP]) bf16: PERSISTENT weight shadows kept by whoever owns the weights
        # (moka_amd.parallel.attach rewrites them behind every optimizer update, one batched launch per gradient bucket).  The forward
        # then launches no moka_weight_shadows and the backward reads these; None: the node computes them per call.
        self.shadows = shadows
        # seed_dev: int64 device tensor of one element the dropout kernels fold into `seed` when they start (moka_opts.seed_dev).  0 in
        # live training (the seed drawn per call is the whole seed); a captured step (schedule.GraphedTrainStep) rewrites it before every
        # replay, so replays of the frozen launch arguments still draw fresh masks.  None: no device part.
        self.seed_dev = seed_dev if self.dropout_p > 0.0 else None


class MokaLinearFn(torch.autograd.Function):
    """(y_0 .. y_{G-1}) = (x W_g^T (+ b_g) + adapter_g(x)) for the G >= 1 projections that read the same x: one projection, q/k/v of
    the attention block, gate/up of the MLP.  x is read once by the G down-projections and once by the G dA kernels, and the G input
    gradients are added to dx in one read-modify-write pass.

    Inputs: x, rt, specs (list of G AdapterSpec: r / s_in / s_out / w / d_k / dropout_p must agree, seeds differ), G, M, then per
    projection W_g, bias_g|None, Bw_g, A_g0..A_g{M-1}.  G = 1 only: fp32 storage, and W_0 = None (the adapter term alone).

    Forward: base GEMMs (hipBLASLt through torch), then the down-projection and either the fused up-projection (+ the weight shadows)
    or the cross-modal interaction and the up-projection, the residual add done in place on the base outputs.  Backward: base
    input-gradient GEMMs (frozen W: no dW), then one pass over gy (dL/dhp and dB), the rank-space backward, and one pass over x / dx
    (dA_m, dx += dh A_m).  Saves x, h and two small operand packs per projection; the softmax is recomputed in rank space.
    """

    @staticmethod
    def forward(ctx, x, rt: MokaRouting, specs, G: int, M: int, *flat):
        per = 3 + M
        Ws, biases, Bws = flat[0::per], flat[1::per], flat[2::per]
        As = [flat[g * per + 3:(g + 1) * per] for g in range(G)]
        _require_device(x, "x")
        no_base = Ws[0] is None                                      # adapter term alone (per-sample adapter_names: several adapters add to one base output)
        if G > 1 and any(W is None for W in Ws):
            raise ValueError("moka_amd: a projection without a base weight (the adapter term alone) is a call of its own, not a member of a group")
        ops, names = [x], ["x"]
        for g in range(G):
            ops += [Bws[g], *As[g]] + ([] if no_base else [Ws[g]])
            names += ["lora_B"] + ["lora_A"] * M + ["base weight"]
        dt = _storage(ops, names)
        bf16 = dt == _lib.MOKA_BF16
        if G > 1 and not bf16:
            raise _lib.MokaError("moka_amd: fp32 storage takes one projection per call (moka_linear_group sends them one at a time)")
        sp = specs[0]
        for o in specs[1:]:
            if (o.r, o.s_in, o.s_out, o.w, o.inv_sqrt_dk, o.dropout_p) != (sp.r, sp.s_in, sp.s_out, sp.w, sp.inv_sqrt_dk, sp.dropout_p) or o.seed_dev is not sp.seed_dev:
                raise ValueError("moka_amd: the projections of one group must share r, scaling, blc/attn weight and dropout")
        if len(sp.s_out) != rt.M or M != rt.M:
            raise ValueError(f"routing describes {rt.M} modalities but {M} adapters / {len(sp.s_out)} scales were given")
        d_in = x.shape[-1]
        x2 = _dense(x.reshape(-1, d_in))
        T, r = x2.shape[0], sp.r
        if T != rt.T:
            raise ValueError(f"x has {T} tokens but the masks describe {rt.T}")
        As = [[_dense(a) for a in Ag] for Ag in As]
        Bws = [_dense(b) for b in Bws]
        need_x = ctx.needs_input_grad[0]
        fused = bf16 and FUSE_FORWARD and _lib.up_fwd_fused_pays(T, _lib.ksplit(T, d_in, r, G), [b.shape[0] for b in Bws], r, dt)
        # persistent (BwT, AT) of the weights' owner, per projection: no launch is then asked for shadows, and none writes into these
        kept = [o.shadows for o in specs] if bf16 and all(o.shadows is not None for o in specs) else None
        if no_base:
            ys = [torch.zeros((T, Bws[0].shape[0]), dtype=x2.dtype, device=x2.device)]
        else:
            ys = [torch.nn.functional.linear(x2, W, b) for W, b in zip(Ws, biases)]      # frozen base, stock PyTorch-ROCm
        parts = down_fwd_group(x2, As, rt, r, sp.s_in, sp.dropout_p, [o.seed for o in specs], sp.seed_dev, dt)
        if not bf16:
            # fp32 storage: the rank-space rows themselves are the operands (no bf16 packs, no weight shadows)
            sts = cross_fwd_group(parts, rt, r, sp.s_out, sp.w, sp.inv_sqrt_dk, want_hp=True)
            hps = sts[0].hp * _token_scale(rt, sp.s_out, x2.device)[:, None]
            up_fwd_group_(ys, [hps], Bws, rt, r, dt)
            sts[0].hp_kmj, sts[0].BwT = hps, Bws[0]                  # what moka_up_bwd takes in their place
        elif fused:
            # two launches on the dependency chain: the up-projection computes the interaction itself from the slices and writes what
            # the backward reads from the rank space (h, hp_kmj); the weight shadows are functions of the weights alone
            sts = up_fwd_fused_group_(ys, parts, Bws, rt, r, sp.s_out, sp.w, sp.inv_sqrt_dk, want_state=True)
            if kept is None:
                BwTs, ATs = weight_shadows_group(Bws, As if need_x else None, r)
                kept = list(zip(BwTs, ATs if ATs is not None else [None] * G))
        else:
            if kept is None:
                sts = cross_fwd_group(parts, rt, r, sp.s_out, sp.w, sp.inv_sqrt_dk, Bws, As if need_x else None)
            else:
                sts = cross_fwd_group(parts, rt, r, sp.s_out, sp.w, sp.inv_sqrt_dk)
            up_fwd_group_(ys, [st.hp_tok for st in sts], Bws, rt, r)
        saved = [x2]
        for g, st in enumerate(sts):
            if kept is not None:
                st.BwT, st.AT = kept[g]
            saved += [Ws[g], Bws[g], st.h, st.hp_kmj, st.BwT, st.AT if need_x else None, *As[g]]
        ctx.save_for_backward(*saved)
        ctx.rt, ctx.specs, ctx.G, ctx.M, ctx.x_shape, ctx.dt = rt, specs, G, M, x.shape, dt
        ctx.has_bias = [b is not None for b in biases]
        return tuple(y.reshape(*x.shape[:-1], y.shape[-1]) for y in ys)

    @staticmethod
    def backward(ctx, *gys):
        G, M, rt, specs, dt = ctx.G, ctx.M, ctx.rt, ctx.specs, ctx.dt
        sp = specs[0]
        r = sp.r
        x2, *saved = ctx.saved_tensors
        per_s = 6 + M
        Ws, Bws, hs, hp_kmjs, BwTs, ATs = (saved[k::per_s] for k in range(6))
        As = [saved[g * per_s + 6:(g + 1) * per_s] for g in range(G)]
        nig = ctx.needs_input_grad
        per, base = 3 + M, 5                                         # x, rt, specs, G, M come first
        if any(nig[base::per]):
            raise _lib.MokaError("moka_amd: the base weight is frozen in MokA; requires_grad on it is not supported")
        dev = x2.device
        T, d_in = x2.shape
        gy2 = []
        for g, t_ in enumerate(gys):
            if t_ is None:                                           # an output that did not reach the loss
                t_ = torch.zeros((T, Bws[g].shape[0]), dtype=x2.dtype, device=dev)
            gy2.append(_dense(t_.reshape(-1, t_.shape[-1])))
        need_x = nig[0]
        on_B = nig[base + 2::per]                                    # per projection: lora_B asked for a gradient
        on_A = [nig[base + g * per + 3:base + (g + 1) * per] for g in range(G)]
        need_B, need_A = any(on_B), any(any(a) for a in on_A)
        use_sinks = all(o.sinks is not None for o in specs)
        if use_sinks:
            # the flat data-parallel gradient buffer is the accumulator (no temporaries, no cast, nothing returned to autograd).  One
            # launch fills the accumulators of the whole group and of ALL modalities: a parameter that asked for no gradient gets a
            # scratch one, so that its sink (somebody else's slice of a flat buffer) keeps its bits
            for g, o in enumerate(specs):
                _check_sinks(o.sinks[0] if need_B else None, list(o.sinks[1]) if need_A else None, Bws[g].shape[0], r, d_in, M, dev)
            shapes, flat = [], None
            acc = ([o.sinks[0] if on_B[g] else torch.zeros_like(o.sinks[0]) for g, o in enumerate(specs)] if need_B else []) + \
                  ([a_ if on_A[g][m] else torch.zeros_like(a_) for g, o in enumerate(specs) for m, a_ in enumerate(o.sinks[1])] if need_A else [])
        else:
            shapes = ([(b.shape[0], r) for b in Bws] if need_B else []) + ([(r, d_in)] * (G * M) if need_A else [])
            flat, acc = _grad_accumulators(shapes, dev) if shapes else (None, [])
        a0 = G if need_B else 0                                      # the accumulators are carved by what is needed: [dB_g ..] [dA_gm ..]
        dB_accs = acc[:G] if need_B else None
        dA_accs = [acc[a0 + g * M:a0 + (g + 1) * M] for g in range(G)] if need_A else None
        defer = sp.defer if use_sinks else None
        described = dt == _lib.MOKA_BF16 and getattr(defer, "accepts_da", False)
        # dB is needed by the optimizer only: where it is a pass of its own over gy anyway (r > 32), it leaves the dependency chain like dA_m
        split_dB = defer is not None and dB_accs is not None and _lib.up_bwd_passes(r, dt) == 2
        g_parts = up_bwd_group(gy2, hp_kmjs, BwTs, rt, r, sp.s_out, None if split_dB else dB_accs, dtype=dt)
        if split_dB:
            fn_db = lambda: up_bwd_group(gy2, hp_kmjs, BwTs, rt, r, sp.s_out, dB_accs, want_g=False, dtype=dt)   # noqa: E731
            if described:
                defer(fn_db, gy2 + list(hp_kmjs), db=((rt, r), list(zip(gy2, hp_kmjs, dB_accs))))
            else:
                defer(fn_db, gy2 + list(hp_kmjs))
        dx2 = None
        if need_x:                                                   # frozen base: dx only, never dW
            dx2 = torch.matmul(gy2[0], Ws[0]) if Ws[0] is not None else torch.zeros_like(x2)
            for g in range(1, G):
                dx2.addmm_(gy2[g], Ws[g])
        if need_A or need_x:
            seeds = [o.seed for o in specs]
            if dt == _lib.MOKA_F32:
                bsts = cross_bwd_group(g_parts, hs, rt, r, sp.s_in, sp.w, sp.inv_sqrt_dk, want_dh=True)
                bsts[0].dh_tok, bsts[0].dh_kmj = bsts[0].dh * sp.s_in, None    # the fp32 rows, scaled, stand in for the packs
                ATs = AT_dA = [torch.stack(list(As[0])).contiguous()]           # ... and the stacked A_m for AT, which the fp32 entry point takes with every call
            else:
                bsts = cross_bwd_group(g_parts, hs, rt, r, sp.s_in, sp.w, sp.inv_sqrt_dk)
                ATs, AT_dA = (ATs if need_x else None), None                   # bf16: the dx half alone reads AT
            if defer is not None and dA_accs is not None:
                if dx2 is not None:
                    down_bwd_group_(bsts, x2, ATs, rt, r, None, dx2, sp.dropout_p, seeds, sp.seed_dev, dt)
                fn = lambda: down_bwd_group_(bsts, x2, AT_dA, rt, r, dA_accs, None, sp.dropout_p, seeds, sp.seed_dev, dt)   # noqa: E731
                keep = [x2] + [b.dh_tok for b in bsts] + [b.dh_kmj for b in bsts] + (AT_dA or [])
                if described:
                    # (described as well: attach() sends a decoder layer's dA_m halves out as ONE launch, moka_down_bwd_da_batch)
                    defer(fn, keep, da=((rt, r, float(sp.dropout_p), sp.seed_dev),
                                        [(bsts[g].dh_kmj, x2, list(dA_accs[g]), seeds[g] or 0) for g in range(G)]))
                else:
                    defer(fn, keep)
            else:
                down_bwd_group_(bsts, x2, ATs, rt, r, dA_accs, dx2, sp.dropout_p, seeds, sp.seed_dev, dt)
        cast = _split_like(flat.to(x2.dtype), shapes) if flat is not None else None      # one cast kernel for all weight gradients
        grads = []
        for g in range(G):
            gbias = gy2[g].sum(0) if (ctx.has_bias[g] and nig[base + g * per + 1]) else None
            gB = cast[g] if (cast and on_B[g]) else None
            gA = [cast[a0 + g * M + m] if (cast and on_A[g][m]) else None for m in range(M)]
            grads += [None, gbias, gB, *gA]
        return (None if dx2 is None else dx2.reshape(ctx.x_shape), None, None, None, None, *grads)


def moka_linear(x, W, bias, Bw, A: Sequence[torch.Tensor], rt: MokaRouting, spec: AdapterSpec):
    if getattr(rt, "dup_src", None) is not None:
        # tokens of several modalities (MokaRouting.from_avt_masks): the adapter term over the real + virtual tokens, the virtual rows folded
        # back onto the tokens they stand for (autograd carries their input gradients the same way); the frozen base sees the real tokens only
        ya = rt.fold(MokaLinearFn.apply(rt.extend(x), rt, [spec], 1, len(A), None, None, Bw, *A)[0]).reshape(*x.shape[:-1], Bw.shape[0])
        return ya if W is None else torch.nn.functional.linear(x, W, bias) + ya
    if getattr(rt, "is_plain", False):                   # mask-free call (masked training calls gather nothing for the decode rule): one launch behind the base GEMM where decode_serves says so
        ys = _decode_forward(x, [(W, bias, Bw, A)], rt, [spec])
        if ys is not None:
            return ys[0]
    return MokaLinearFn.apply(x, rt, [spec], 1, len(A), W, bias, Bw, *A)[0]


def moka_linear_group(x, projections, rt: MokaRouting, specs: Sequence[AdapterSpec]):
    """projections: list of (W, bias|None, Bw, [A_0..A_{M-1}]) fed by the same x.  Returns the list of outputs."""
    if x.dtype == torch.float32 or getattr(rt, "dup_src", None) is not None:          # fp32 storage / virtual tokens: correctness paths, one projection at a time
        return [moka_linear(x, W, b, Bw, A, rt, sp) for (W, b, Bw, A), sp in zip(projections, specs)]
    if getattr(rt, "is_plain", False):                                                   # (see moka_linear)
        ys = _decode_forward(x, projections, rt, list(specs))
        if ys is not None:
            return ys
    G = len(projections)
    M = len(projections[0][3])
    flat = []
    for W, b, Bw, A in projections:
        flat += [W, b, Bw, *A]
    return list(MokaLinearFn.apply(x, rt, list(specs), G, M, *flat))
