#!/usr/bin/env python
"""Cached decode steps of a MokaLlamaStack, timed four ways in ONE process (needs an MI355X; fails loudly without one):

    merged   MokaLlamaStack.merge_for_decode(): one GEMM per projection, no adapter work -- the floor
    old      functional.DECODE_FORWARD = False: the autograd nodes' forward (the training launch chain) on a handful of tokens
    new      functional.DECODE_FORWARD = True:  base GEMMs + one moka_decode_fwd launch per projection group
    fused    functional.DLINEAR_FORWARD = True: one moka_dlinear_fwd launch per projection group, the base GEMV inside (T <= 16; above
             it the calls fall through to the `old` path)

    python tools/decode_step.py [--dims 7b|13b] [--r 16] [--layers 32] [--prefill 2048] [--batches 1,4,16]
                                [--steps 200] [--warmup 20] [--repeats 3] [--mode all|merged|old|new|fused] [--out FILE]

The modes alternate in blocks (warm-up + timed steps each) and the whole alternation is repeated, so that drifts of the box hit all four
alike; a mode's figure is the median of its blocks, its spread their max - min.  Steps are timed with device events around a block and
are what a caller of the stack sees (host launch cost included); ``graph_ms`` is the same step captured into a graph and replayed -- the
device-side cost alone.  adapter ms = mode - merged.  ``projection_launches_per_step`` = base GEMM calls (torch.nn.functional.linear) + decode /
fused kernel launches + general-path entry-point calls (each of those is at least one launch: a lower bound for `old`).
``fused_beats_decode_kernel`` uses the criterion of ``new_beats_old``: the difference is larger than the larger of the two spreads;
``fused_over_merged`` is the ratio of the step times, ``merged_copy_bytes`` the second dense copy of the projection weights the merged
mode holds and the fused mode does not need.  One JSON line (appended to --out when given, always printed).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DIMS = {"7b": dict(hidden=4096, ff=11008, n_heads=32, n_kv_heads=32), "13b": dict(hidden=5120, ff=13824, n_heads=40, n_kv_heads=40)}
MODES = ("merged", "old", "new", "fused")


def build_stack(dims, layers, r, dev):
    from moka_amd.decoder import LlamaDims, MokaLlamaStack
    from moka_amd.peft_hyper import Linear

    def make(d_in, d_out):
        m = Linear(d_in, d_out, r=(r, r, r), lora_alpha=16, lora_nums=3, blc_weight=1.0, blc_alpha=1, lora_dropout=0.0,
                   loramethod="test", bias=False, device=dev, dtype=torch.bfloat16)
        torch.nn.init.normal_(m.lora_B0.weight, std=0.05)
        return m

    return MokaLlamaStack(LlamaDims(**dims), layers, make).to(dev, torch.bfloat16).eval()


def avt_masks(B, S, dev):
    """[text, video, audio, question]: S/32 text, S/2 video, S/8 audio, S/32 question tokens, the rest text (64 / 1024 / 256 / 64 of 2048)."""
    if S < 32:
        raise SystemExit("tools/decode_step.py: --prefill must be at least 32")
    t0, v, a, nq = S // 32, S // 2, S // 8, S // 32
    tok = torch.zeros(S, dtype=torch.long)
    tok[t0:t0 + v] = 1
    tok[t0 + v:t0 + v + a] = 2
    q = torch.zeros(S, dtype=torch.int32)
    q[t0 + v + a:t0 + v + a + nq] = 1
    ms = [(tok == m).to(torch.int32).reshape(1, S, 1).repeat(B, 1, 1).to(dev) for m in range(3)]
    return ms + [q.reshape(1, S, 1).repeat(B, 1, 1).to(dev)]


def count_general_calls(F, fn):
    """(entry-point calls of the general path, torch.nn.functional.linear calls) during fn() (each is at least one launch)."""
    names = ["down_fwd", "down_fwd_group", "cross_fwd", "cross_fwd_group", "up_fwd_", "up_fwd_group_", "up_fwd_fused_", "up_fwd_fused_group_",
             "weight_shadows", "weight_shadows_group"]
    n, nlin = [0], [0]
    saved = {k: getattr(F, k) for k in names}
    linear = torch.nn.functional.linear

    def counted_linear(*a, **kw):
        nlin[0] += 1
        return linear(*a, **kw)

    def wrap(f):
        def g(*a, **kw):
            n[0] += 1
            return f(*a, **kw)
        return g

    for k, f in saved.items():
        setattr(F, k, wrap(f))
    torch.nn.functional.linear = counted_linear
    try:
        fn()
    finally:
        torch.nn.functional.linear = linear
        for k, f in saved.items():
            setattr(F, k, f)
    return n[0], nlin[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="7b", choices=sorted(DIMS))
    ap.add_argument("--r", type=int, default=16)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--prefill", type=int, default=2048)
    ap.add_argument("--batches", default="1,4,16")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--mode", default="all", choices=("all",) + MODES)
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/decode_step.py needs an MI355X: no ROCm device is visible")
    from moka_amd import _decode_lib, _dlinear_lib, functional as F
    _decode_lib.load()
    _dlinear_lib.load()
    dev = torch.device("cuda:0")
    modes = MODES if args.mode == "all" else (args.mode,)
    torch.manual_seed(0)
    st = build_stack(DIMS[args.dims], args.layers, args.r, dev)
    hidden = DIMS[args.dims]["hidden"]
    result = {"tool": "decode_step", "dims": args.dims, "layers": args.layers, "r": args.r, "prefill": args.prefill, "steps": args.steps,
              "warmup": args.warmup, "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
              "decode_max_tokens": int(_decode_lib.load().moka_decode_max_tokens()),
              "dlinear_max_tokens": int(_dlinear_lib.load().moka_dlinear_max_tokens()), "batches": {}}

    def set_mode(mode):
        F.DECODE_FORWARD = mode == "new"
        F.DLINEAR_FORWARD = mode == "fused"
        if mode == "merged":
            if getattr(st, "_merged", None) is None:
                st.merge_for_decode()
        else:
            st.unmerge()

    saved = (F.DECODE_FORWARD, F.DLINEAR_FORWARD)
    try:
        with torch.no_grad():
            for B in [int(b) for b in args.batches.split(",")]:
                masks = avt_masks(B, args.prefill, dev)
                h = torch.randn(B, args.prefill, hidden, device=dev).to(torch.bfloat16)
                tok = torch.randn(B, 1, hidden, device=dev).to(torch.bfloat16)
                st.unmerge()
                _, caches = st(h, masks)
                del h
                step = lambda: st(tok, masks, kv_caches=caches)[0]      # noqa: E731  (the cache is not grown: every step is the same work)
                blocks = {m: [] for m in modes}
                for _ in range(args.repeats):
                    for mode in modes:
                        set_mode(mode)
                        for _ in range(args.warmup):
                            step()
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(args.steps):
                            step()
                        e1.record()
                        e1.synchronize()
                        blocks[mode].append(e0.elapsed_time(e1) / args.steps)
                entry = {}
                for mode in modes:
                    set_mode(mode)
                    n0, d0 = F.decode_launches, F.dlinear_launches
                    calls, gemms = count_general_calls(F, step)
                    entry[mode] = {"ms": statistics.median(blocks[mode]), "spread_ms": max(blocks[mode]) - min(blocks[mode]), "blocks_ms": blocks[mode],
                                   "decode_launches_per_step": F.decode_launches - n0, "dlinear_launches_per_step": F.dlinear_launches - d0,
                                   "general_path_calls_per_step": calls, "base_gemm_calls_per_step": gemms}
                    entry[mode]["projection_launches_per_step"] = (gemms + calls + entry[mode]["decode_launches_per_step"]
                                                                   + entry[mode]["dlinear_launches_per_step"])
                    if mode == "merged":
                        result["merged_copy_bytes"] = sum(w.numel() * w.element_size() for w, _ in st._merged.values())
                    if not args.no_graph:
                        try:
                            torch.cuda.synchronize()
                            graph = torch.cuda.CUDAGraph()
                            with torch.cuda.graph(graph):
                                step()
                            for _ in range(args.warmup):
                                graph.replay()
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record()
                            for _ in range(args.steps):
                                graph.replay()
                            e1.record()
                            e1.synchronize()
                            entry[mode]["graph_ms"] = e0.elapsed_time(e1) / args.steps
                            del graph
                        except Exception as e:                            # a mode that does not capture: reported, not fatal
                            entry[mode]["graph_ms"] = None
                            entry[mode]["graph_error"] = str(e).splitlines()[0][:200]
                            torch.cuda.synchronize()
                if "merged" in entry:
                    for mode in modes:
                        if mode != "merged":
                            entry[mode]["adapter_ms"] = entry[mode]["ms"] - entry["merged"]["ms"]
                            if entry[mode].get("graph_ms") is not None and entry["merged"].get("graph_ms") is not None:
                                entry[mode]["adapter_graph_ms"] = entry[mode]["graph_ms"] - entry["merged"]["graph_ms"]
                if "old" in entry and "new" in entry and "merged" in entry:
                    gain = entry["old"]["adapter_ms"] - entry["new"]["adapter_ms"]
                    entry["new_beats_old"] = bool(gain > max(entry["old"]["spread_ms"], entry["new"]["spread_ms"]))
                if "new" in entry and "fused" in entry:
                    gain = entry["new"]["ms"] - entry["fused"]["ms"]
                    entry["fused_beats_decode_kernel"] = bool(gain > max(entry["new"]["spread_ms"], entry["fused"]["spread_ms"]))
                if "merged" in entry and "fused" in entry:
                    entry["fused_over_merged"] = entry["fused"]["ms"] / entry["merged"]["ms"]
                result["batches"][str(B)] = entry
                print(f"B={B}: " + ", ".join(f"{m} {entry[m]['ms']:.3f} ms (spread {entry[m]['spread_ms']:.3f}, graph {entry[m].get('graph_ms')})" for m in modes),
                      file=sys.stderr, flush=True)
                del caches, masks
                torch.cuda.empty_cache()
    finally:
        F.DECODE_FORWARD, F.DLINEAR_FORWARD = saved
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
