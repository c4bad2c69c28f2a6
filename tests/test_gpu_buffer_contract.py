"""The buffer contract of every product kernel form (include/moka_hip.h), checked through the C ABI with every caller-owned buffer
in a guard-banded arena (tests/arena.py), against the fp64 oracle.  The routing arrays (tok_mod, ktok, klen, kslot) are the one
exception: they stay in the routing object's own allocations (their padding past T is part of the contract) and are checked
unchanged after every call.

tests/kernel_forms.py lists every kernel instance of the library (tests/test_kernel_forms_host.py keeps it in step with the built
library); that the rows reach every one of them is shown by a
kernel trace of this file:  rocprofv3 --kernel-trace --stats -- python -m pytest tests/test_gpu_buffer_contract.py -m gpu

One row per kernel form: a shape with tails (T % 16, T % 32, T % 128 != 0 where the form allows; widths with C % 128 in {32, 96},
C % 512 != 0), routing whose spans start and end inside 16- and 32-token tiles, tokens of no modality.  Each row runs the whole
adapter pipeline (down_fwd -> cross_fwd + up_fwd or up_fwd_fused + weight_shadows -> up_bwd -> cross_bwd -> down_bwd), one entry
point at a time, each call with its own arena:
  * outputs start as NaN and must be written in full; documented padding (rank columns r..RP, pack tokens T..Tp, other modalities'
    tokens of a dh_kmj plane, BwT / AT pad) must be exactly zero;
  * accumulators (dA_acc, dB_acc) and the in/out y / dx start at seeded finite values of the increment's magnitude: the increment is
    what is compared with the oracle, so a form that overwrites fails; rows of tokens of no modality keep their bits;
  * workspaces (cross backward, deterministic mode) start as garbage;
  * guards and inputs are bit-identical afterwards.
Tolerances are those of tests/test_gpu_parity.py::_stage_check.  Every row runs twice: buffers on 256-byte boundaries, then -- once that
has passed -- 144 bytes past them (16-byte aligned only), where an entry point either gives results that pass the same checks or
refuses the alignment with MOKA_EINVAL.
"""
import math
from ctypes import byref, c_float, c_int, c_ulonglong, c_void_p

import pytest
import torch

from oracle import cases as C
from oracle import moka_oracle as O
from tests.arena import Arena, Buf
from tests.test_gpu_parity import TOL_BF16, TOL_F32, _check_routing, rel, ulp_bf16_diff

pytestmark = pytest.mark.gpu

bf, f32 = torch.bfloat16, torch.float32
SHIFTS = (0, 144)
EINVAL = -1


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _lib():
    from moka_amd import _lib as L
    return L


def _stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def _vp(ptrs):
    return (c_void_p * len(ptrs))(*ptrs)


def _fl(vals):
    return (c_float * len(vals))(*[float(v) for v in vals])


def _in(vals):
    return (c_int * len(vals))(*[int(v) for v in vals])


def _u64(vals):
    return (c_ulonglong * len(vals))(*[int(v) for v in vals])


def _kmj_index(RP, Tp):
    """[RP, Tp] flat offset of (rank k, token t) inside one plane of the *_kmj layout (include/moka_hip.h)."""
    tt = torch.arange(Tp)
    tl = tt % 32
    p = torch.where(tl < 16, 8 * (tl // 4) + tl % 4, 8 * ((tl - 16) // 4) + 4 + tl % 4)
    kk = torch.arange(RP).reshape(RP, 1)
    return ((kk // 16) * (Tp // 32) + (tt // 32).reshape(1, Tp)) * 512 + ((kk % 16) + 16 * (p // 8).reshape(1, Tp)) * 8 + (p % 8).reshape(1, Tp)


def _kmj_zero(RP, Tp, keep):
    """Bool mask of a [.., RP*Tp] plane that must be zero: every (rank, token) outside `keep` [RP, Tp]."""
    z = torch.ones(RP * Tp, dtype=torch.bool)
    z[_kmj_index(RP, Tp).reshape(-1)[keep.reshape(-1)]] = False
    return z


def _kmj_read(plane_pair, RP, Tp):
    """hi + lo of a plane pair [2, RP*Tp] in (rank, token) order."""
    off = _kmj_index(RP, Tp).reshape(-1)
    flat = plane_pair.float().cpu().reshape(2, -1)
    return (flat[0] + flat[1])[off].reshape(RP, Tp)


class Call:
    """One entry-point call in its own arena.  At shift != 0 the only accepted alternative to a passing call is MOKA_EINVAL for an
    alignment requirement (the row then goes on with the results of the default placement); any other refusal fails.  The routing
    arrays are the routing object's own device buffers, not arena buffers: they are checked unchanged after every call."""
    rt = None

    def __init__(self, what, spec, fn, shift, seed=0):
        self.what = what
        before = _routing_bits(Call.rt)
        a = Arena(_dev(), spec, shift=shift, seed=seed)
        rc = fn(a)
        if rc == EINVAL and shift:
            msg = _lib().load().moka_last_error().decode()
            assert "align" in msg, f"{what} at +{shift} B: MOKA_EINVAL that is not an alignment requirement: {msg}"
            a = Arena(_dev(), spec, shift=0, seed=seed)
            rc = fn(a)
        assert rc == 0, f"{what}: rc={rc} {_lib().load().moka_last_error().decode()}"
        torch.cuda.synchronize()
        a.check()
        assert _routing_bits(Call.rt) == before, f"{what}: the routing arrays changed"
        self.a = a

    def __getitem__(self, name):
        return self.a.view(name)


def _routing_bits(rt):
    if rt is None:
        return None
    return [t.cpu().numpy().tobytes() for t in (rt.tok_mod, rt.ktok, rt.klen, rt.kslot)]


def _routing(variant, B, S, layouts):
    from moka_amd.routing import MokaRouting
    tm, qq = zip(*[C.build_layout(l_, S) for l_ in layouts])
    tok_mod, question = torch.stack(tm), torch.stack(qq)
    dev = _dev()
    if variant == "avt":
        masks = [(tok_mod == m).to(torch.int32).unsqueeze(-1) for m in range(3)] + [question.to(torch.int32).unsqueeze(-1)]
        rt, ort = MokaRouting.from_avt_masks([m.to(dev) for m in masks]), O.routing_from_avt_masks(masks)
    else:
        masks = [tok_mod == 0, tok_mod == 1, question]
        rt, ort = MokaRouting.from_vt_masks(*[m.to(dev) for m in masks]), O.routing_from_vt_masks(*masks)
    _check_routing(rt, ort)
    Call.rt = rt
    return rt, ort


def _tiled_layout(S, kinds="tvaq", spans=(13, 7, 29, 5, 18, 3, 45, 11, 22, 9), lead=("p", 5)):
    """Spans that start and end inside 16- and 32-token tiles, padding inside and at the end."""
    lay, left, k = [lead], S - lead[1], 0
    while left > 0:
        n = min(spans[k % len(spans)], left)
        kind = kinds[k % len(kinds)] if k % 11 != 10 else "p"
        lay.append((kind, n))
        left -= n
        k += 1
    if not any(kd == "q" for kd, _ in lay):
        lay[2] = ("q", lay[2][1])
    return lay


def _bf(t):
    return t.to(bf).float()


def _data(cfg):
    """Inputs (bf16-representable fp32 on the host) of a row."""
    r, d_in, d_outs, B, S = cfg["r"], cfg["d_in"], cfg["d_outs"], cfg["B"], cfg["S"]
    M = 3 if cfg["variant"] == "avt" else 2
    g = torch.Generator().manual_seed(cfg.get("seed", 0) + 1000)
    T = B * S
    x = _bf(torch.randn(T, d_in, generator=g))
    A = [[_bf((torch.rand(r, d_in, generator=g) * 2 - 1) / math.sqrt(d_in)) for _ in range(M)] for _ in d_outs]
    Bw = [_bf(torch.randn(d, r, generator=g) * 0.05) for d in d_outs]
    gy = [_bf(torch.randn(T, d, generator=g)) for d in d_outs]
    return x, A, Bw, gy, g


def _prior_like(t, g, scale=None):
    """Seeded finite prior of an accumulator / in-out buffer with the magnitude of the increment it will receive."""
    s = float(t.double().pow(2).mean().sqrt()) if scale is None else scale
    return torch.randn(t.shape, generator=g) * (s if s > 0 else 1.0)


def _keep_masks(cfg, T, d_in, shift):
    """Per projection: the keep mask (moka_dropout_mask, itself in an arena) and 1/(1-p')."""
    L = _lib()
    lib = L.load()
    p = cfg.get("p", 0.0)
    if p == 0:
        return [None] * len(cfg["d_outs"]), [0] * len(cfg["d_outs"]), 1.0
    seeds = [0xC0FFEE + 977 * i for i in range(len(cfg["d_outs"]))]
    keeps = []
    for s in seeds:
        c = Call("moka_dropout_mask", {"keep": Buf((T, d_in), torch.uint8, "write")},
                 lambda a, s=s: lib.moka_dropout_mask(float(p), s, T, d_in, a.ptr("keep"), _stream()), shift)
        k = c["keep"].cpu()
        assert int((k > 1).sum()) == 0
        keeps.append(k.double())
    return keeps, seeds, float(lib.moka_dropout_scale(float(p)))


def _pipeline(cfg, shift):
    L = _lib()
    lib = L.load()
    r, d_in, d_outs, B, S, variant = cfg["r"], cfg["d_in"], list(cfg["d_outs"]), cfg["B"], cfg["S"], cfg["variant"]
    G, T = len(d_outs), B * S
    M = 3 if variant == "avt" else 2
    RP, Tp = L.rank_pad(r), L.tok_pad(T)
    layouts = cfg.get("layouts") or [_tiled_layout(S, "tvaq" if variant == "avt" else "tvq", lead=("p", 5 + 3 * b)) for b in range(B)]
    rt, ort = _routing(variant, B, S, layouts)
    if variant == "avt":
        s_in, s_out, w = 16.0 / r, [1.0] * 3, 1.0
    else:
        s_in, s_out, w = 1.0, [16.0 / r] * 2, 0.05
    c_sm = 1.0 / math.sqrt(r)
    x, A, Bw, gy, gen = _data(cfg)
    tm = ort.tok_mod.reshape(T)
    valid, none = tm >= 0, tm < 0
    keeps, seeds, inv_keep = _keep_masks(cfg, T, d_in, shift)
    p = cfg.get("p", 0.0)

    # ---------- oracle, per projection (fp64)
    scale = torch.zeros(T, 1, dtype=torch.float64)
    for m in range(M):
        scale[tm == m] = s_out[m]
    ora = []
    dx_term = torch.zeros(T, d_in, dtype=torch.float64)
    for g in range(G):
        xm = x.double() if keeps[g] is None else x.double() * keeps[g] * inv_keep
        yo, ctx = O.adapter_forward(xm.reshape(B, S, d_in), torch.zeros(B, S, d_outs[g]), A[g], Bw[g], ort, s_in, s_out, w, r)
        dxm, dAo, dBo, dho = O.adapter_backward(gy[g].reshape(B, S, -1), ctx)
        dxm = dxm.reshape(T, d_in)
        dx_term += dxm if keeps[g] is None else dxm * keeps[g] * inv_keep
        gpo = (gy[g].double() * scale) @ Bw[g].double()
        ora.append(dict(h=ctx.h.reshape(T, r), hp=ctx.hp.reshape(T, r), y=yo.reshape(T, -1), dA=dAo, dB=dBo, dh=dho.reshape(T, r), g=gpo))
    y0 = [_bf(_prior_like(o["y"], gen)) for o in ora]
    dx0 = _bf(_prior_like(dx_term, gen))
    Aflat = [a for Ag in A for a in Ag]

    # ---------- down-projection (moka_down_fwd_group)
    ks = L.ksplit(T, d_in, r, G)
    part_exempt = none.reshape(1, T, 1).expand(ks, T, RP)
    spec = {"x": Buf((T, d_in), bf, "input", data=x)}
    spec.update({f"A{i}": Buf((r, d_in), bf, "input", data=a) for i, a in enumerate(Aflat)})
    spec.update({f"part{g}": Buf((ks, T, RP), f32, "write", exempt=part_exempt) for g in range(G)})
    c = Call("moka_down_fwd_group", spec, lambda a: lib.moka_down_fwd_group(
        a.ptr("x"), _vp([a.ptr(f"A{i}") for i in range(G * M)]), rt.tok_mod.data_ptr(), _vp([a.ptr(f"part{g}") for g in range(G)]),
        T, d_in, r, M, G, s_in, float(p), _u64(seeds), L.MOKA_BF16, None, _stream()), shift)
    parts = []
    for g in range(G):
        pt = c[f"part{g}"].cpu().clone()
        assert rel(pt.sum(0)[:, :r][valid], ora[g]["h"][valid]) < TOL_F32, f"down_fwd part{g}"
        parts.append(pt)

    # ---------- forward: up_fwd_fused + weight_shadows, or cross_fwd + up_fwd
    fused = cfg.get("fused")
    if fused is None:
        fused = L.up_fwd_fused_pays(T, ks, d_outs, r)
    rank_zero = torch.zeros(T, RP, dtype=torch.bool)
    rank_zero[:, r:] = True
    tok_zero = torch.zeros(Tp, 2 * RP, dtype=torch.bool)
    tok_zero[:, r:RP] = tok_zero[:, RP + r:] = True
    tok_zero[T:] = True
    live = torch.zeros(RP, Tp, dtype=torch.bool)
    live[:r, :T] = valid.reshape(1, T)
    kmj_zero = _kmj_zero(RP, Tp, live).reshape(1, -1).expand(2, -1)
    spec = {f"part{g}": Buf((ks, T, RP), f32, "input", data=parts[g]) for g in range(G)}
    spec.update({f"Bw{g}": Buf((d_outs[g], r), bf, "input", data=Bw[g]) for g in range(G)})
    spec.update({f"y{g}": Buf((T, d_outs[g]), bf, "inout", data=y0[g]) for g in range(G)})
    spec.update({f"h{g}": Buf((T, RP), f32, "write", zero=rank_zero) for g in range(G)})
    spec.update({f"hp_kmj{g}": Buf((2, RP * Tp), bf, "write", zero=kmj_zero, flat=True) for g in range(G)})
    if fused:
        c = Call("moka_up_fwd_fused_group", spec, lambda a: lib.moka_up_fwd_fused_group(
            _vp([a.ptr(f"part{g}") for g in range(G)]), ks, byref(rt.struct), _fl(s_out), _vp([a.ptr(f"Bw{g}") for g in range(G)]),
            _vp([a.ptr(f"y{g}") for g in range(G)]), _in(d_outs), _vp([a.ptr(f"h{g}") for g in range(G)]),
            _vp([a.ptr(f"hp_kmj{g}") for g in range(G)]), G, r, w, c_sm, L.MOKA_BF16, _stream()), shift)
        ys = [c[f"y{g}"].cpu() for g in range(G)]
    else:
        for g in range(G):
            del spec[f"y{g}"]
            spec[f"hp{g}"] = Buf((T, RP), f32, "write", zero=rank_zero)
            spec[f"hp_tok{g}"] = Buf((Tp, 2 * RP), bf, "write", zero=tok_zero)
        c = Call("moka_cross_fwd_group", spec, lambda a: lib.moka_cross_fwd_group(
            _vp([a.ptr(f"part{g}") for g in range(G)]), ks, byref(rt.struct), _fl(s_out), _vp([a.ptr(f"Bw{g}") for g in range(G)]),
            _in(d_outs), None, d_in, _vp([a.ptr(f"h{g}") for g in range(G)]), _vp([a.ptr(f"hp{g}") for g in range(G)]),
            _vp([a.ptr(f"hp_tok{g}") for g in range(G)]), _vp([a.ptr(f"hp_kmj{g}") for g in range(G)]), None, None,
            G, r, w, c_sm, _stream()), shift)
        hp_toks = [c[f"hp_tok{g}"].cpu().clone() for g in range(G)]
        for g in range(G):
            assert rel(c[f"hp{g}"][:, :r].cpu(), ora[g]["hp"]) < TOL_F32, f"cross_fwd hp{g}"
            tp = hp_toks[g].float()
            assert rel((tp[:T, :RP] + tp[:T, RP:])[:, :r], ora[g]["hp"] * scale) < TOL_F32, f"hp_tok{g}"
        spec2 = {f"hp_tok{g}": Buf((Tp, 2 * RP), bf, "input", data=hp_toks[g]) for g in range(G)}
        spec2.update({f"Bw{g}": Buf((d_outs[g], r), bf, "input", data=Bw[g]) for g in range(G)})
        spec2.update({f"y{g}": Buf((T, d_outs[g]), bf, "inout", data=y0[g]) for g in range(G)})
        cy = Call("moka_up_fwd_group", spec2, lambda a: lib.moka_up_fwd_group(
            _vp([a.ptr(f"hp_tok{g}") for g in range(G)]), _vp([a.ptr(f"Bw{g}") for g in range(G)]), rt.tok_mod.data_ptr(),
            _vp([a.ptr(f"y{g}") for g in range(G)]), T, r, _in(d_outs), G, L.MOKA_BF16, _stream()), shift)
        ys = [cy[f"y{g}"].cpu() for g in range(G)]
    hs = [c[f"h{g}"].cpu().clone() for g in range(G)]
    hp_kmjs = [c[f"hp_kmj{g}"].cpu().clone() for g in range(G)]
    for g in range(G):
        assert rel(hs[g][:, :r], ora[g]["h"]) < TOL_F32, f"h{g}"
        kmj = _kmj_read(hp_kmjs[g], RP, Tp)
        assert rel(kmj[:r, :T].t(), ora[g]["hp"] * scale) < TOL_F32, f"hp_kmj{g}"
        y_exact = (y0[g].double() + ora[g]["y"]).to(bf)
        assert rel(ys[g], y_exact) < TOL_BF16, f"y{g}"
        assert ulp_bf16_diff(ys[g], y_exact, y0[g]) <= 1.0 + 1e-6, f"y{g} ulp"
        assert torch.equal(ys[g][none], y0[g].to(bf)[none]), f"y{g}: rows of no modality changed"

    # ---------- weight shadows (moka_weight_shadows_group)
    bwt_zero = torch.zeros(RP, 1, dtype=torch.bool)
    bwt_zero[r:] = True
    at_zero = torch.zeros(1, 1, RP, dtype=torch.bool)
    at_zero[..., r:] = True
    spec = {f"Bw{g}": Buf((d_outs[g], r), bf, "input", data=Bw[g]) for g in range(G)}
    spec.update({f"A{i}": Buf((r, d_in), bf, "input", data=a) for i, a in enumerate(Aflat)})
    spec.update({f"BwT{g}": Buf((RP, d_outs[g]), bf, "write", zero=bwt_zero.expand(RP, d_outs[g])) for g in range(G)})
    spec.update({f"AT{g}": Buf((M, d_in, RP), bf, "write", zero=at_zero.expand(M, d_in, RP)) for g in range(G)})
    c = Call("moka_weight_shadows_group", spec, lambda a: lib.moka_weight_shadows_group(
        _vp([a.ptr(f"Bw{g}") for g in range(G)]), _in(d_outs), _vp([a.ptr(f"A{i}") for i in range(G * M)]), d_in,
        _vp([a.ptr(f"BwT{g}") for g in range(G)]), _vp([a.ptr(f"AT{g}") for g in range(G)]), G, r, M, _stream()), shift)
    BwTs = [c[f"BwT{g}"].cpu().clone() for g in range(G)]
    ATs = [c[f"AT{g}"].cpu().clone() for g in range(G)]
    for g in range(G):
        assert torch.equal(BwTs[g][:r], Bw[g].to(bf).t()), f"BwT{g}"
        for m in range(M):
            assert torch.equal(ATs[g][m, :, :r], A[g][m].to(bf).t()), f"AT{g}"

    # ---------- up-projection backward (moka_up_bwd_group; dB alone when it is a pass of its own)
    Cmax = max(d_outs)
    ksb = L.ksplit_bwd(T, Cmax, r)
    two_pass = L.up_bwd_passes(r) == 2
    det = cfg.get("det", False)
    dB0 = [_prior_like(o["dB"], gen).float() for o in ora]

    def det_opts(a, n):
        return byref(L.MokaOpts(a.ptr("det_ws"), n)) if det else None

    def up_bwd_spec(with_g, with_db, det_fill):
        sp = {f"gy{g}": Buf((T, d_outs[g]), bf, "input", data=gy[g]) for g in range(G)}
        sp.update({f"hp_kmj{g}": Buf((2, RP * Tp), bf, "input", data=hp_kmjs[g], flat=True) for g in range(G)})
        sp.update({f"BwT{g}": Buf((RP, d_outs[g]), bf, "input", data=BwTs[g]) for g in range(G)})
        if with_g:
            sp.update({f"g_part{g}": Buf((ksb, T, RP), f32, "write", exempt=none.reshape(1, T, 1).expand(ksb, T, RP)) for g in range(G)})
        if with_db:
            sp.update({f"dB{g}": Buf((d_outs[g], r), f32, "inout", data=dB0[g]) for g in range(G)})
            if det:
                sp["det_ws"] = Buf((int(lib.moka_deterministic_ws_bytes(T, Cmax, r, G, M)),), torch.uint8, "workspace", fill=det_fill)
        return sp

    def up_bwd(a, with_g, with_db):
        return lib.moka_up_bwd_group(
            _vp([a.ptr(f"gy{g}") for g in range(G)]), _vp([a.ptr(f"hp_kmj{g}") for g in range(G)]), _vp([a.ptr(f"BwT{g}") for g in range(G)]),
            rt.tok_mod.data_ptr(), _fl(s_out), _vp([a.ptr(f"g_part{g}") for g in range(G)]) if with_g else None,
            _vp([a.ptr(f"dB{g}") for g in range(G)]) if with_db else None, T, r, _in(d_outs), M, G, L.MOKA_BF16,
            det_opts(a, a.spec["det_ws"].numel) if (det and with_db) else None, _stream())

    def db_batch(a):
        return lib.moka_up_bwd_db_batch(
            _vp([a.ptr(f"gy{g}") for g in range(G)]), _vp([a.ptr(f"hp_kmj{g}") for g in range(G)]), _in(d_outs), rt.tok_mod.data_ptr(),
            _vp([a.ptr(f"dB{g}") for g in range(G)]), G, T, r, M, L.MOKA_BF16, det_opts(a, a.spec["det_ws"].numel) if det else None, _stream())

    if two_pass or cfg.get("split_bwd"):     # g alone, then dB as a pass of its own (moka_up_bwd_passes() == 2, or a caller that splits them)
        c = Call("moka_up_bwd_group (g)", up_bwd_spec(True, False, "garbage"), lambda a: up_bwd(a, True, False), shift)
        db_what, db_with_g = ("moka_up_bwd_db_batch", False) if cfg.get("db_batch") else ("moka_up_bwd_group (dB)", False)
        db_fn = db_batch if cfg.get("db_batch") else (lambda a: up_bwd(a, False, True))
        cb = Call(db_what, up_bwd_spec(False, True, "garbage"), db_fn, shift)
    else:                                    # one pass over gy for both
        db_what, db_with_g = "moka_up_bwd_group", True
        db_fn = lambda a: up_bwd(a, True, True)      # noqa: E731
        c = cb = Call(db_what, up_bwd_spec(True, True, "garbage"), db_fn, shift)
    g_parts = [c[f"g_part{g}"].cpu().clone() for g in range(G)]
    for g in range(G):
        assert rel(g_parts[g].sum(0)[:, :r][valid], ora[g]["g"][valid]) < TOL_F32, f"up_bwd g{g}"
        cb.a.check_delta(f"dB{g}", ora[g]["dB"], TOL_F32)
    if det:                                  # the same call on a zeroed workspace: the same bits
        ref = Call(db_what + " (zeroed det_ws)", up_bwd_spec(db_with_g, True, "zero"), db_fn, shift)
        for g in range(G):
            assert torch.equal(ref[f"dB{g}"].cpu(), cb[f"dB{g}"].cpu()), f"dB{g}: the deterministic mode depends on the workspace's prior contents"

    # ---------- interaction backward (moka_cross_bwd_group), workspaces of garbage
    ws_n = int(lib.moka_cross_ws_bytes(B, S, rt.Lk_max, r))
    dh_zero = torch.zeros(T, RP, dtype=torch.bool)
    dh_zero[:, r:] = True
    dtok_zero = tok_zero
    kmj_planes = []
    for m in range(M):
        lv = torch.zeros(RP, Tp, dtype=torch.bool)
        lv[:r, :T] = (tm == m).reshape(1, T)
        kmj_planes.append(_kmj_zero(RP, Tp, lv).reshape(1, -1).expand(2, -1))
    dkmj_zero = torch.stack(kmj_planes)
    spec = {f"g_part{g}": Buf((ksb, T, RP), f32, "input", data=g_parts[g]) for g in range(G)}
    spec.update({f"h{g}": Buf((T, RP), f32, "input", data=hs[g]) for g in range(G)})
    spec.update({f"dh{g}": Buf((T, RP), f32, "write", zero=dh_zero) for g in range(G)})
    spec.update({f"dh_tok{g}": Buf((Tp, 2 * RP), bf, "write", zero=dtok_zero) for g in range(G)})
    spec.update({f"dh_kmj{g}": Buf((M, 2, RP * Tp), bf, "write", zero=dkmj_zero) for g in range(G)})
    spec.update({f"ws{g}": Buf((ws_n,), torch.uint8, "workspace") for g in range(G)})
    c = Call("moka_cross_bwd_group", spec, lambda a: lib.moka_cross_bwd_group(
        _vp([a.ptr(f"g_part{g}") for g in range(G)]), ksb, _vp([a.ptr(f"h{g}") for g in range(G)]), byref(rt.struct), s_in,
        _vp([a.ptr(f"dh{g}") for g in range(G)]), _vp([a.ptr(f"dh_tok{g}") for g in range(G)]), _vp([a.ptr(f"dh_kmj{g}") for g in range(G)]),
        _vp([a.ptr(f"ws{g}") for g in range(G)]), G, r, w, c_sm, _stream()), shift)
    dh_toks = [c[f"dh_tok{g}"].cpu().clone() for g in range(G)]
    dh_kmjs = [c[f"dh_kmj{g}"].cpu().clone() for g in range(G)]
    for g in range(G):
        assert rel(c[f"dh{g}"][:, :r].cpu()[valid], ora[g]["dh"][valid]) < TOL_F32, f"cross_bwd dh{g}"
        dt = dh_toks[g].float()
        assert rel((dt[:T, :RP] + dt[:T, RP:])[:, :r][valid], s_in * ora[g]["dh"][valid]) < TOL_F32, f"dh_tok{g}"
        for m in range(M):
            sel = tm == m
            if bool(sel.any()):
                kmj = _kmj_read(dh_kmjs[g][m], RP, Tp)
                assert rel(kmj[:r, :T].t()[sel], s_in * ora[g]["dh"][sel]) < TOL_F32, f"dh_kmj{g} plane {m}"

    # ---------- down-projection backward: dA (moka_down_bwd_group or moka_down_bwd_da_batch) and dx
    dA0 = [[_prior_like(ora[g]["dA"][m], gen).float() for m in range(M)] for g in range(G)]
    da_batch = cfg.get("da_batch", False)

    def down_spec(with_da, with_dx, det_fill):
        sp = {"x": Buf((T, d_in), bf, "input", data=x)}
        sp.update({f"dh_tok{g}": Buf((Tp, 2 * RP), bf, "input", data=dh_toks[g]) for g in range(G)})
        sp.update({f"dh_kmj{g}": Buf((M, 2, RP * Tp), bf, "input", data=dh_kmjs[g]) for g in range(G)})
        sp.update({f"AT{g}": Buf((M, d_in, RP), bf, "input", data=ATs[g]) for g in range(G)})
        if with_da:
            sp.update({f"dA{g}_{m}": Buf((r, d_in), f32, "inout", data=dA0[g][m]) for g in range(G) for m in range(M)})
            if det:
                sp["det_ws"] = Buf((int(lib.moka_deterministic_ws_bytes(T, d_in, r, G, M)),), torch.uint8, "workspace", fill=det_fill)
        if with_dx:
            sp["dx"] = Buf((T, d_in), bf, "inout", data=dx0)
        return sp

    def down_bwd(a, with_da, with_dx):
        if with_da and da_batch:
            return lib.moka_down_bwd_da_batch(
                _vp([a.ptr(f"dh_kmj{g}") for g in range(G)]), _vp([a.ptr("x")] * G), _in([d_in] * G), rt.tok_mod.data_ptr(),
                _vp([a.ptr(f"dA{g}_{m}") for g in range(G) for m in range(M)]), G, T, r, M, float(p), _u64(seeds), L.MOKA_BF16,
                det_opts(a, a.spec["det_ws"].numel) if det else None, _stream())
        return lib.moka_down_bwd_group(
            _vp([a.ptr(f"dh_tok{g}") for g in range(G)]), _vp([a.ptr(f"dh_kmj{g}") for g in range(G)]), a.ptr("x"),
            _vp([a.ptr(f"AT{g}") for g in range(G)]), rt.tok_mod.data_ptr(),
            _vp([a.ptr(f"dA{g}_{m}") for g in range(G) for m in range(M)]) if with_da else None, a.ptr("dx") if with_dx else None,
            T, d_in, r, M, G, float(p), _u64(seeds), L.MOKA_BF16, det_opts(a, a.spec["det_ws"].numel) if (det and with_da) else None, _stream())

    if da_batch:
        cdx = Call("moka_down_bwd_group (dx)", down_spec(False, True, "garbage"), lambda a: down_bwd(a, False, True), shift)
        cda = Call("moka_down_bwd_da_batch", down_spec(True, False, "garbage"), lambda a: down_bwd(a, True, False), shift)
    else:
        cdx = cda = Call("moka_down_bwd_group", down_spec(True, True, "garbage"), lambda a: down_bwd(a, True, True), shift)
    for g in range(G):
        for m in range(M):
            cda.a.check_delta(f"dA{g}_{m}", ora[g]["dA"][m], TOL_F32)
    dx = cdx["dx"].cpu()
    dx_exact = (dx0.double() + dx_term).to(bf)
    assert rel(dx, dx_exact) < TOL_BF16, "dx"
    assert ulp_bf16_diff(dx, dx_exact, dx0) <= 1.0 + 1e-6, "dx ulp"
    assert torch.equal(dx[none], dx0.to(bf)[none]), "dx: rows of no modality changed"
    if det:
        ref = Call("down_bwd dA (det, zeroed ws)", down_spec(True, False, "zero"), lambda a: down_bwd(a, True, False), shift)
        for g in range(G):
            for m in range(M):
                assert torch.equal(ref[f"dA{g}_{m}"].cpu(), cda[f"dA{g}_{m}"].cpu()), f"dA{g}_{m}: deterministic mode depends on the workspace"


# One row per kernel form.  `forms`: what the row is meant to reach (the instance names of the product build; the selecting rule in
# comments).  Shapes: T % 16 != 0 unless the form needs whole 16-token tiles, C % 128 in {32, 96}, C % 512 != 0.
ROWS = [
    # -- down-projection, rank pad 16
    # mk_launch_down_fwd (T % 16 == 0) -> moka_xs_kernel<G>; gs<16, dB> (launch_gy); fused yx<16> (moka_up_fwd_fused_pays: C <= 6144);
    #    moka_expand_kernel<16, 4, false, 1, false> dx; moka_wgrad_kernel RP 16, C <= 8192
    dict(id="xs1_yx16_r16", variant="avt", r=16, B=2, S=520, d_in=1376, d_outs=(1120,), p=0.1),
    # moka_xs_kernel<2>; moka_expand_kernel<16, 2, false, 2, false> dx; wgrad G = 2; fused group (moka_up_fwd_fused_pays: G > 1)
    dict(id="xs2_group_r16", variant="vt", r=12, B=2, S=272, d_in=1120, d_outs=(1376, 1376)),
    # moka_xs_kernel<3>; wgrad G = 3; up_fwd two-launch, unequal widths (fused_pays: widths differ)
    dict(id="xs3_unequal_r16", variant="avt", r=16, B=1, S=1040, d_in=1376, d_outs=(1120, 352, 160), det=True),
    # launch_xa: moka_xa_kernel<1, 2> (G == 1, C > 8192, T % 16 != 0); wgrad RP 16 with C > 8192 (4-wave form)
    dict(id="xa1_wide_r16", variant="avt", r=16, B=1, S=1001, d_in=8224, d_outs=(1120,), p=0.1),
    # moka_xa_kernel<2, 4>
    dict(id="xa2_r16", variant="vt", r=16, B=3, S=333, d_in=1376, d_outs=(352, 1120), p=0.1),
    # moka_xa_kernel<3, 8>; moka_yt_kernel<16> (batched equal widths, two-launch forced); cross_bwd on long key lists
    dict(id="xa3_yt16_r16", variant="avt", r=16, B=2, S=1037, d_in=1376, d_outs=(1120, 1120, 1120), fused=False),
    # single projection C > 6144: cross_fwd + moka_expand_kernel<16, ...> (moka_up_fwd_fused_pays)
    dict(id="expand16_single_wide", variant="avt", r=16, B=1, S=999, d_in=1120, d_outs=(6240,)),
    # launch_gy: moka_gy_kernel (rank pad 16, nz > 1, Cmax > 8192, T > 4096): gate + up 2 x 11008 at 4130 tokens, dropout
    dict(id="gy16_gate_up", variant="avt", r=16, B=2, S=2065, d_in=1376, d_outs=(11008, 11008), p=0.1, layouts=None),
    # -- rank pad 32
    # moka_xwm_kernel<32, false, 1>; gs<32, dB>; fused yx<32>; moka_expand_kernel<32, 4, false, 1, true> dx; wgrad RP 32
    dict(id="xwm32_g1", variant="avt", r=24, B=1, S=1001, d_in=1376, d_outs=(1120,), p=0.1),
    # moka_xwm_kernel<32, false, 2>; moka_dxgt_kernel<32, 2>; yt<32> (two-launch, equal widths)
    dict(id="xwm32_g2_yt32", variant="vt", r=32, B=2, S=333, d_in=1376, d_outs=(1120, 1120), fused=False),
    # moka_xwm_kernel<32, false, 3>, unequal widths (slices of the narrow members are tails); moka_dxgt_kernel<32, 3>; zbatch dA
    dict(id="xwm32_g3_unequal", variant="avt", r=32, B=1, S=1001, d_in=1376, d_outs=(1120, 352, 96), da_batch=True, p=0.1),
    # -- rank pad 64
    # moka_xwm_kernel<64, false, 1>; g: moka_xwm_kernel<64, true, 1> + separate dB pass (moka_up_bwd_passes == 2); yt<64>; moka_dxt_kernel<64>;
    # moka_wgrad_wide_kernel<., false>
    dict(id="xwm64_g1", variant="avt", r=48, B=1, S=1001, d_in=1376, d_outs=(1120,), p=0.1),
    # moka_xwm_kernel<64, false, 2>; moka_dxgt_kernel<64, 2>; moka_up_bwd_db_batch; wide wgrad zbatch
    dict(id="xwm64_g2_dbbatch", variant="vt", r=64, B=2, S=333, d_in=1376, d_outs=(1120, 352), db_batch=True, da_batch=True),
    # moka_xwm_kernel<64, false, 3>; moka_dxgt_kernel<64, 3>; deterministic wide wgrad + moka_sum_runs_kernel
    dict(id="xwm64_g3_det", variant="avt", r=64, B=1, S=1001, d_in=1376, d_outs=(1120, 352, 160), det=True),
    # deterministic RP 16 single projection with dropout (moka_wgrad_kernel<..., true>, gs<16, dB, det>)
    dict(id="det_r16", variant="vt", r=16, B=2, S=333, d_in=1376, d_outs=(1120,), det=True, p=0.1),


    # -- forms the rows above miss (moka_hip.h: every output may be requested alone; the deterministic mode at every rank pad)
    # launch_gy NG = 16: 44 active 512-column blocks x 256 token groups x 1/16 >= 2 x 256 CUs -- gate + up at 8190 tokens, the e2e shape
    #    -> moka_gy_kernel<true, 16, false>; with det_ws moka_gy_kernel<true, 16, true>
    dict(id="gy16_gate_up_8k", variant="avt", r=16, B=2, S=4095, d_in=160, d_outs=(11008, 11008), shifts=(0,)),
    dict(id="gy16_gate_up_8k_det", variant="avt", r=16, B=2, S=4095, d_in=160, d_outs=(11008, 11008), det=True, p=0.1, shifts=(0,)),
    # launch_gy NG = 8 with det_ws -> moka_gy_kernel<true, 8, true>
    dict(id="gy16_gate_up_det", variant="avt", r=16, B=2, S=2065, d_in=160, d_outs=(11008, 11008), det=True, shifts=(0,)),
    # g alone (launch_gy: 4 groups without dB) -> moka_gy_kernel<false, 4, false>; dB alone through moka_up_bwd_db_batch with det_ws
    #    (one moka_up_bwd per problem) -> moka_wgrad_kernel<16, 8, true, 1, true>; dA det of a pair -> moka_wgrad_kernel<16, 4, false, 2, true>
    dict(id="gy16_gate_up_det_split", variant="avt", r=16, B=2, S=2065, d_in=160, d_outs=(11008, 11008), det=True, split_bwd=True, db_batch=True,
         shifts=(0,)),
    # rank pad 16, g and dB in separate calls: moka_gs_kernel<16, false, false>; moka_wgrad_kernel<16, 8, true, 1, false> (launch_wgrad)
    dict(id="split_r16", variant="avt", r=16, B=1, S=1001, d_in=1376, d_outs=(1120,), split_bwd=True),
    # det dA of a wide input (launch_wgrad, C > 8192) -> moka_wgrad_kernel<16, 4, false, 1, true>
    dict(id="det_r16_wide", variant="avt", r=16, B=1, S=333, d_in=8224, d_outs=(160,), det=True),
    # rank pad 32 det: moka_gs_kernel<32, true, true>, moka_wgrad_kernel<32, 8, false, 1, true>
    dict(id="det_r32", variant="avt", r=32, B=1, S=1001, d_in=1376, d_outs=(1120,), det=True, p=0.1),
    # rank pad 32, g and dB in separate calls: moka_gs_kernel<32, false, false>; moka_wgrad_kernel<32, 8, true, 1, false>
    dict(id="split_r32", variant="vt", r=24, B=2, S=333, d_in=1376, d_outs=(1120,), split_bwd=True),
    # ... dB through moka_up_bwd_db_batch with det_ws -> moka_wgrad_kernel<32, 8, true, 1, true>
    dict(id="split_r32_det", variant="avt", r=32, B=1, S=1001, d_in=1376, d_outs=(1120, 352), split_bwd=True, db_batch=True, det=True),
    # moka_up_fwd_fused at rank pad 64 (valid; moka_up_fwd_fused_pays advises against it) -> moka_yx_kernel<64>
    dict(id="yx64_fused", variant="avt", r=64, B=1, S=1001, d_in=1376, d_outs=(1120,), fused=True),
]

_PASSED_256 = set()


@pytest.mark.parametrize("cfg,shift", [(c_, s_) for c_ in ROWS for s_ in c_.get("shifts", SHIFTS)],
                         ids=[f"{c_['id']}-{s_}" for c_ in ROWS for s_ in c_.get("shifts", SHIFTS)])
def test_kernel_form(cfg, shift):
    """The 16-byte placement of a row runs only after its 256-byte placement has passed (in this test or an earlier one).  The rows
    of the largest shapes run at the default placement only: their entry points are covered at 16 bytes by the smaller rows."""
    cfg = dict(cfg)
    cfg["seed"] = sum(ord(ch) for ch in cfg["id"])
    if shift and cfg["id"] not in _PASSED_256:
        _pipeline(cfg, 0)
        _PASSED_256.add(cfg["id"])
    _pipeline(cfg, shift)
    if not shift:
        _PASSED_256.add(cfg["id"])


# ------------------------------------------------------------------------------------------
# fp32 storage (MOKA_F32): moka_f32_reduce_kernel, moka_f32_expand_kernel, moka_f32_wgrad_kernel, one projection at a time
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("det", [False, True])
def test_fp32_storage_forms(shift, det):
    L = _lib()
    lib = L.load()
    r, B, S, d_in, d_out, p = 12, 1, 333, 352, 160, 0.1
    T, M = B * S, 3
    RP = L.rank_pad(r)
    rt, ort = _routing("avt", B, S, [_tiled_layout(S)])
    s_in, s_out = 16.0 / r, [1.0, 1.0, 1.0]
    g = torch.Generator().manual_seed(71)
    x = torch.randn(T, d_in, generator=g)
    A = [(torch.rand(r, d_in, generator=g) * 2 - 1) / math.sqrt(d_in) for _ in range(M)]
    Bw = torch.randn(d_out, r, generator=g) * 0.05
    gy = torch.randn(T, d_out, generator=g)
    tm = ort.tok_mod.reshape(T)
    valid, none = tm >= 0, tm < 0
    seed = 4242
    ck = Call("moka_dropout_mask", {"keep": Buf((T, d_in), torch.uint8, "write")},
              lambda a: lib.moka_dropout_mask(p, seed, T, d_in, a.ptr("keep"), _stream()), shift)
    keep, inv_keep = ck["keep"].cpu().double(), float(lib.moka_dropout_scale(p))
    xm = x.double() * keep * inv_keep
    yo, ctx = O.adapter_forward(xm.reshape(B, S, d_in), torch.zeros(B, S, d_out), A, Bw, ort, s_in, s_out, 1.0, r)
    dxm, dAo, dBo, dho = O.adapter_backward(gy.reshape(B, S, d_out), ctx)
    h, hp, dh = ctx.h.reshape(T, r), ctx.hp.reshape(T, r), dho.reshape(T, r)
    scale = (tm >= 0).double().reshape(T, 1)
    tol = 1e-5
    # down_fwd: moka_f32_reduce_kernel
    ks = L.ksplit(T, d_in, r)
    spec = {"x": Buf((T, d_in), f32, "input", data=x), **{f"A{m}": Buf((r, d_in), f32, "input", data=A[m]) for m in range(M)},
            "part": Buf((ks, T, RP), f32, "write", exempt=none.reshape(1, T, 1).expand(ks, T, RP))}
    c = Call("moka_down_fwd f32", spec, lambda a: lib.moka_down_fwd(a.ptr("x"), _vp([a.ptr(f"A{m}") for m in range(M)]), rt.tok_mod.data_ptr(),
                                                                   a.ptr("part"), T, d_in, r, M, s_in, p, seed, L.MOKA_F32, None, _stream()), shift)
    assert rel(c["part"].cpu().sum(0)[:, :r][valid], h[valid]) < tol
    # up_fwd: moka_f32_expand_kernel (hp_tok = s_out[mod] * hp, fp32 [T, RP])
    hp_rows = torch.zeros(T, RP)
    hp_rows[:, :r] = (hp * scale).float()
    y0 = _prior_like(yo.reshape(T, d_out), g).float()
    spec = {"hp": Buf((T, RP), f32, "input", data=hp_rows), "Bw": Buf((d_out, r), f32, "input", data=Bw), "y": Buf((T, d_out), f32, "inout", data=y0)}
    c = Call("moka_up_fwd f32", spec, lambda a: lib.moka_up_fwd(a.ptr("hp"), a.ptr("Bw"), rt.tok_mod.data_ptr(), a.ptr("y"), T, r, d_out, L.MOKA_F32, _stream()), shift)
    c.a.check_delta("y", yo.reshape(T, d_out), tol)
    assert torch.equal(c["y"].cpu()[none], y0[none])
    # up_bwd: g (moka_f32_reduce_kernel, shared weights) and dB (moka_f32_wgrad_kernel [+ moka_sum_runs_kernel])
    ksb = L.ksplit_bwd(T, d_out, r)
    dB0 = _prior_like(dBo, g).float()
    nws = int(lib.moka_deterministic_ws_bytes(T, d_out, r, 1, M))
    spec = {"gy": Buf((T, d_out), f32, "input", data=gy), "hp": Buf((T, RP), f32, "input", data=hp_rows), "Bw": Buf((d_out, r), f32, "input", data=Bw),
            "g_part": Buf((ksb, T, RP), f32, "write", exempt=none.reshape(1, T, 1).expand(ksb, T, RP)), "dB": Buf((d_out, r), f32, "inout", data=dB0)}
    if det:
        spec["det_ws"] = Buf((nws,), torch.uint8, "workspace")
    c = Call("moka_up_bwd f32", spec, lambda a: lib.moka_up_bwd(a.ptr("gy"), a.ptr("hp"), a.ptr("Bw"), rt.tok_mod.data_ptr(), _fl(s_out), a.ptr("g_part"),
                                                               a.ptr("dB"), T, r, d_out, M, L.MOKA_F32,
                                                               byref(L.MokaOpts(a.ptr("det_ws"), nws)) if det else None, _stream()), shift)
    gpo = (gy.double() * scale) @ Bw.double()
    assert rel(c["g_part"].cpu().sum(0)[:, :r][valid], gpo[valid]) < tol
    c.a.check_delta("dB", dBo, tol)
    # down_bwd: dA (moka_f32_wgrad_kernel) and dx (moka_f32_expand_kernel); dh_tok = s_in * dh fp32 [T, RP], AT = the A_m stacked
    dh_rows = torch.zeros(T, RP)
    dh_rows[:, :r] = (s_in * dh * scale).float()
    dA0 = [_prior_like(dAo[m], g).float() for m in range(M)]
    dx0 = _prior_like(dxm.reshape(T, d_in), g).float()
    nws = int(lib.moka_deterministic_ws_bytes(T, d_in, r, 1, M))
    spec = {"dh": Buf((T, RP), f32, "input", data=dh_rows), "x": Buf((T, d_in), f32, "input", data=x),
            "AT": Buf((M, r, d_in), f32, "input", data=torch.stack(A)), "dx": Buf((T, d_in), f32, "inout", data=dx0),
            **{f"dA{m}": Buf((r, d_in), f32, "inout", data=dA0[m]) for m in range(M)}}
    if det:
        spec["det_ws"] = Buf((nws,), torch.uint8, "workspace")
    c = Call("moka_down_bwd f32", spec, lambda a: lib.moka_down_bwd(a.ptr("dh"), None, a.ptr("x"), a.ptr("AT"), rt.tok_mod.data_ptr(),
                                                                   _vp([a.ptr(f"dA{m}") for m in range(M)]), a.ptr("dx"), T, d_in, r, M, p, seed,
                                                                   L.MOKA_F32, byref(L.MokaOpts(a.ptr("det_ws"), nws)) if det else None, _stream()), shift)
    for m in range(M):
        c.a.check_delta(f"dA{m}", dAo[m], tol)
    c.a.check_delta("dx", dxm.reshape(T, d_in) * keep * inv_keep, tol)
    assert torch.equal(c["dx"].cpu()[none], dx0[none])


# ------------------------------------------------------------------------------------------
# the other kernels
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("r", [12, 20, 48])
def test_weight_shadows_single_and_batch(r, shift):
    """moka_weight_shadows and moka_weight_shadows_batch (widths of every tail): BwT / AT pad exactly zero, the rest the transposes."""
    L = _lib()
    lib = L.load()
    M = 3
    RP = L.rank_pad(r)
    g = torch.Generator().manual_seed(5)
    widths = [(96, 160), (1120, 352), (32, 1376)]
    Bws = [_bf(torch.randn(do, r, generator=g)) for do, _ in widths]
    As = [[_bf(torch.randn(r, di, generator=g)) for _ in range(M)] for _, di in widths]
    spec = {}
    for i, (do, di) in enumerate(widths):
        z_b = torch.zeros(RP, do, dtype=torch.bool)
        z_b[r:] = True
        z_a = torch.zeros(M, di, RP, dtype=torch.bool)
        z_a[..., r:] = True
        spec[f"Bw{i}"] = Buf((do, r), bf, "input", data=Bws[i])
        spec.update({f"A{i}_{m}": Buf((r, di), bf, "input", data=As[i][m]) for m in range(M)})
        spec[f"BwT{i}"] = Buf((RP, do), bf, "write", zero=z_b)
        spec[f"AT{i}"] = Buf((M, di, RP), bf, "write", zero=z_a)
    n = len(widths)
    c = Call("moka_weight_shadows_batch", spec, lambda a: lib.moka_weight_shadows_batch(
        _vp([a.ptr(f"Bw{i}") for i in range(n)]), _in([w_[0] for w_ in widths]), _vp([a.ptr(f"A{i}_{m}") for i in range(n) for m in range(M)]),
        _in([w_[1] for w_ in widths]), _vp([a.ptr(f"BwT{i}") for i in range(n)]), _vp([a.ptr(f"AT{i}") for i in range(n)]), n, r, M, _stream()), shift)
    for i in range(n):
        assert torch.equal(c[f"BwT{i}"][:r].cpu(), Bws[i].to(bf).t())
        for m in range(M):
            assert torch.equal(c[f"AT{i}"][m, :, :r].cpu(), As[i][m].to(bf).t())
    one = {k: v for k, v in spec.items() if k.endswith("2") or k.startswith("A2_")}
    c1 = Call("moka_weight_shadows", one, lambda a: lib.moka_weight_shadows(
        a.ptr("Bw2"), widths[2][0], _vp([a.ptr(f"A2_{m}") for m in range(M)]), widths[2][1], a.ptr("BwT2"), a.ptr("AT2"), r, M, _stream()), shift)
    assert torch.equal(c1["BwT2"].cpu(), c["BwT2"].cpu()) and torch.equal(c1["AT2"].cpu(), c["AT2"].cpu())


@pytest.mark.parametrize("shift", SHIFTS)
def test_dropout_mask_fills_exactly_its_extent(shift):
    """keep_out of T * d_in bytes, T * d_in not a multiple of 16: every byte 0 / 1, none past the end; the rate is p."""
    lib = _lib().load()
    T, d_in, p = 333, 40, 0.1
    c = Call("moka_dropout_mask", {"keep": Buf((T, d_in), torch.uint8, "write")},
             lambda a: lib.moka_dropout_mask(p, 99, T, d_in, a.ptr("keep"), _stream()), shift)
    k = c["keep"].cpu()
    assert int((k > 1).sum()) == 0
    assert abs(1 - k.double().mean().item() - p) < 4 * math.sqrt(p * (1 - p) / k.numel())


@pytest.mark.parametrize("dev_coef", [False, True])
def test_adamw_on_a_ragged_slice(dev_coef):
    """moka_adamw_flat / moka_adamw_flat_dev on the slice [lo, hi) of the five flat buffers (hi ragged): nothing outside the slice
    changes, the slice matches torch.optim.AdamW; moka_adamw_begin_dev writes exactly its 8 floats."""
    L = _lib()
    lib = L.load()
    dev = _dev()
    n, lo, hi = 10007, 1024, 9001
    lr, b1, b2, eps, wd, step = 1e-3, 0.9, 0.999, 1e-8, 0.01, 3
    g = torch.Generator().manual_seed(8)
    master = torch.randn(n, generator=g)
    grad = torch.randn(n, generator=g)
    m0 = torch.randn(n, generator=g) * 0.1
    v0 = torch.rand(n, generator=g) * 0.01
    spec = {"master": Buf((n,), f32, "inout", data=master), "work": Buf((n,), bf, "inout", data=master),
            "grad": Buf((n,), f32, "inout", data=grad), "m": Buf((n,), f32, "inout", data=m0), "v": Buf((n,), f32, "inout", data=v0)}
    if dev_coef:
        spec["state8"] = Buf((8,), f32, "write", exempt=torch.arange(8) == 7)        # [7]: not part of the contract
    a = Arena(dev, spec)

    def sl(name):
        return a.view(name)[lo:].data_ptr()
    if dev_coef:
        L.check(lib.moka_adamw_begin_dev(a.ptr("state8"), lr, b1, b2, wd, step, _stream()), "moka_adamw_begin_dev")
        rc = lib.moka_adamw_flat_dev(sl("master"), sl("work"), sl("grad"), sl("m"), sl("v"), hi - lo, b1, b2, eps, a.ptr("state8"), 0.5, 1, _stream())
    else:
        rc = lib.moka_adamw_flat(sl("master"), sl("work"), sl("grad"), sl("m"), sl("v"), hi - lo, lr, b1, b2, eps, wd, step, 0.5, 1, _stream())
    assert rc == 0, lib.moka_last_error().decode()
    torch.cuda.synchronize()
    if dev_coef:
        st = a.view("state8").cpu()
        c3 = (c_float * 3)()
        lib.moka_adamw_coef(lr, b1, b2, wd, step, c3)
        assert st[:3].tolist() == pytest.approx(list(c3), rel=1e-6) and int(st[3:4].view(torch.int32)) == step
    a.check()
    outside = torch.ones(n, dtype=torch.bool)
    outside[lo:hi] = False
    for name in ("master", "grad", "m", "v", "work"):
        assert torch.equal(a.view(name).cpu()[outside], a.prior(name).cpu()[outside]), f"{name} changed outside the slice"
    assert float(a.view("grad")[lo:hi].abs().max()) == 0.0                       # zero_grad
    p = torch.nn.Parameter(master[lo:hi].clone().double())
    opt = torch.optim.AdamW([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    opt.state[p] = {"step": torch.tensor(float(step - 1)), "exp_avg": m0[lo:hi].double().clone(), "exp_avg_sq": v0[lo:hi].double().clone()}
    p.grad = grad[lo:hi].double() * 0.5
    opt.step()
    assert rel(a.view("master")[lo:hi], p.detach()) < 1e-6
    assert rel(a.view("m")[lo:hi], opt.state[p]["exp_avg"]) < 1e-6
    assert rel(a.view("v")[lo:hi], opt.state[p]["exp_avg_sq"]) < 1e-6
    assert torch.equal(a.view("work")[lo:hi].cpu(), a.view("master")[lo:hi].cpu().to(bf))


def test_guards_see_a_row_written_past_a_short_extent():
    """moka_up_fwd over T rows while the arena declares y one row short: the last row lands in the guard band (inside the allocation)
    and the arena reports exactly that row -- the guards work on the device."""
    L = _lib()
    lib = L.load()
    r, B, S, d_out = 16, 1, 77, 160
    T = B * S
    RP, Tp = L.rank_pad(r), L.tok_pad(T)
    rt, ort = _routing("avt", B, S, [[("p", 3), ("t", 30), ("v", 20), ("q", 10), ("t", 14)]])
    g = torch.Generator().manual_seed(12)
    pack = torch.zeros(Tp, 2 * RP)
    pack[:T, :r] = _bf(torch.randn(T, r, generator=g))
    Bw = _bf(torch.randn(d_out, r, generator=g))
    y0 = _bf(torch.randn(T - 1, d_out, generator=g))
    a = Arena(_dev(), {"hp_tok": Buf((Tp, 2 * RP), bf, "input", data=pack), "Bw": Buf((d_out, r), bf, "input", data=Bw),
                       "y": Buf((T - 1, d_out), bf, "inout", data=y0)})
    assert lib.moka_up_fwd(a.ptr("hp_tok"), a.ptr("Bw"), rt.tok_mod.data_ptr(), a.ptr("y"), T, r, d_out, L.MOKA_BF16, _stream()) == 0
    torch.cuda.synchronize()
    dmg = a.guard_damage()
    assert len(dmg) == 1, dmg
    name, side, first, last = dmg[0]
    assert (name, side) == ("y", "after") and first // d_out == 0 and last // d_out == 0, dmg      # row T-1 and nothing else
    assert "y: written past the end" in "; ".join(a.problems())
