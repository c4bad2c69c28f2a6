"""Data parallelism of the adapter WITH the kernels: two ranks share the one GPU of the box (gloo
stages the gradient buckets through the host -- a functional check of the N > 1 path, never a measurement), each runs
the forward + backward of a small adapted decoder stack on its half of the batch through ``moka_amd.parallel.attach``
(weight-gradient kernels accumulating straight into the flat bucket, all-reduce fired from the decoder layers' backward
hooks); the averaged flat gradient must equal the gradient of the mean loss over the whole batch computed by ONE rank.

Tolerance: the two computations sum the same fp32 products in a different order (atomics across blocks, per-sample vs
batched launches): <= 2e-4 relative on the flat gradient.  With the bf16 all-reduce payload every rank's contribution
and the sum are rounded to 8 bits of mantissa (2^-9 each, relative to terms that partly cancel across samples): <= 2e-2.
"""
import os
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _build(variant, dev, rank=8):
    from moka_amd.decoder import LlamaDims, MokaLlamaStack
    dims = LlamaDims(hidden=256, ff=512, n_heads=4, n_kv_heads=4)
    torch.manual_seed(11)
    if variant == "avt":
        from moka_amd.peft_hyper import Linear

        def make(d_in, d_out):
            m = Linear(d_in, d_out, r=(rank, rank, rank), lora_alpha=16, lora_nums=3, blc_weight=1.0, blc_alpha=1, lora_dropout=0.0,
                       loramethod="train", bias=False)
            torch.nn.init.normal_(m.weight, std=0.05)
            torch.nn.init.normal_(m.lora_B0.weight, std=0.05)
            return m
    else:
        from moka_amd.modified_peft import Linear

        def make(d_in, d_out):
            base = torch.nn.Linear(d_in, d_out, bias=False)
            torch.nn.init.normal_(base.weight, std=0.05)
            m = Linear(base, "image", r=rank, lora_alpha=16, lora_dropout=0.0, attn_weight=0.05)
            m.update_layer("text", rank, lora_alpha=16, lora_dropout=0.0, init_lora_weights=True, use_rslora=False)
            m.set_adapter(["image", "text"])
            for n in ("image", "text"):
                torch.nn.init.normal_(m.lora_B[n].weight, std=0.05)
            return m
    st = MokaLlamaStack(dims, 3, make).to(dev, torch.bfloat16).train()
    for n, p in st.named_parameters():
        p.requires_grad = "lora_" in n
    return st, dims


def _batch(variant, dims, dev, B=2, S=96):
    g = torch.Generator().manual_seed(5)
    h = torch.randn(B, S, dims.hidden, generator=g).to(dev, torch.bfloat16)
    gout = torch.randn(B, S, dims.hidden, generator=g).to(dev, torch.bfloat16)
    tok = torch.zeros(B, S, dtype=torch.int64)
    tok[:, 4:36] = 1
    q = torch.zeros(B, S, dtype=torch.bool)
    q[0, 60:72] = True
    q[1, 58:75] = True
    if variant == "avt":
        tok[:, 40:56] = 2
        masks = [(tok == m).to(torch.int32).unsqueeze(-1).to(dev) for m in range(3)] + [q.to(torch.int32).unsqueeze(-1).to(dev)]
        return h, gout, (masks,), lambda lo, hi: ([m[lo:hi] for m in masks],)
    masks = [(tok == 0).to(dev), (tok == 1).to(dev), q.to(dev)]
    return h, gout, tuple(masks), lambda lo, hi: tuple(m[lo:hi] for m in masks)


def _run(st, dp, h, gout, mask_args, scale):
    out, _ = st(h, *mask_args)
    (out.float() * gout.float()).sum().mul(scale).backward()


def _worker(rank, world, port, variant, comm_bf16, q):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from moka_amd.parallel import attach
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    st, dims = _build(variant, dev)
    dp = attach(st, n_buckets=2, comm_dtype=torch.bfloat16 if comm_bf16 else None)
    h, gout, _, sl = _batch(variant, dims, dev)
    _run(st, dp, h[rank:rank + 1], gout[rank:rank + 1], sl(rank, rank + 1), 1.0)      # my sample; mean over samples = average over ranks
    dp.finish(average=True)
    torch.cuda.synchronize()
    before = dp.work.clone()
    dp.bucket.flat.mul_(world)                                                      # step() averages itself
    dp.step()
    torch.cuda.synchronize()
    q.put((rank, dp.bucket.flat.abs().max().item(), (dp.work.float() - before.float()).abs().max().item()))
    # (gradients were consumed by step(); recompute them for the comparison)
    _run(st, dp, h[rank:rank + 1], gout[rank:rank + 1], sl(rank, rank + 1), 1.0)
    dp.finish(average=True)
    torch.cuda.synchronize()
    q.put((rank, "grad", dp.bucket.flat.cpu().numpy(), list(dp.names), list(dp.offsets)))   # by value (the process exits)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("variant,comm_bf16", [("avt", False), ("vt", False), ("avt", True)])
def test_two_ranks_average_equals_the_full_batch_gradient(variant, comm_bf16):
    assert torch.cuda.is_available()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, variant, comm_bf16, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = {}
    steps = []
    for _ in range(4):
        item = q.get(timeout=240)
        if item[1] == "grad":
            got[item[0]] = item[2:]
        else:
            steps.append(item)
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    # the optimizer step left zeroed gradients and moved the bf16 parameters
    for _, gmax, moved in steps:
        assert gmax == 0.0 and moved > 0.0
    # single rank, whole batch, mean loss over the two samples
    from moka_amd.parallel import attach
    dev = torch.device("cuda:0")
    st, dims = _build(variant, dev)
    dp = attach(st, n_buckets=2)
    before = dp.work.clone()
    h, gout, mask_args, _ = _batch(variant, dims, dev)
    # rank-side state after ONE optimizer step: replay that step here so that the second gradient is taken at the same weights
    _run(st, dp, h, gout, mask_args, 0.5)
    dp.step()
    assert (dp.work.float() - before.float()).abs().max().item() > 0
    _run(st, dp, h, gout, mask_args, 0.5)
    dp.finish(average=True)
    torch.cuda.synchronize()
    ref = dp.bucket.flat.cpu()
    tol = 2e-2 if comm_bf16 else 2e-4
    for r in (0, 1):
        flat, names, offsets = got[r]
        flat = torch.from_numpy(flat)
        assert names == dp.names and offsets == dp.offsets
        err = ((flat - ref).norm() / ref.norm()).item()
        assert err <= tol, (r, err)
    assert (got[0][0] == got[1][0]).all(), "both ranks must hold the same averaged gradient"
    assert ref.norm().item() > 0


def test_attach_feeds_the_kernels_and_matches_plain_autograd():
    """World 1: gradients through the sinks of attach() == the gradients the autograd nodes return without it (cast to bf16)."""
    dev = torch.device("cuda:0")
    from moka_amd.parallel import attach
    st_a, dims = _build("avt", dev)
    st_b, _ = _build("avt", dev)
    h, gout, mask_args, _ = _batch("avt", dims, dev)
    _run(st_b, None, h, gout, mask_args, 1.0)
    dp = attach(st_a, n_buckets=3)
    _run(st_a, dp, h, gout, mask_args, 1.0)
    dp.finish(average=True)
    torch.cuda.synchronize()
    pb = dict(st_b.named_parameters())
    n_checked = 0
    for n, o in zip(dp.names, dp.offsets):
        p = pb[n]
        assert dict(st_a.named_parameters())[n].grad is None          # autograd carries no adapter gradient
        g_flat = dp.bucket.flat[o:o + p.numel()].view(p.shape)
        if p.grad is None:
            continue
        err = ((g_flat - p.grad.float()).norm() / p.grad.float().norm().clamp_min(1e-20)).item()
        assert err <= 6e-3, (n, err)                                  # p.grad went through a bf16 cast
        n_checked += 1
    assert n_checked == 3 * 7 * 4
    # layer grouping: offsets ascend layer by layer, every layer's hook fired (all buckets were shipped by the hooks)
    assert dp.bucket.n_layers == 3


def test_two_half_batches_on_two_streams_add_up_to_the_full_batch():
    """The samples of a micro-batch are independent chains of launches (nothing in the model mixes tokens of different samples):
    half the batch on each of two HIP streams, forward + backward through the kernels CONCURRENTLY, the weight-gradient kernels of
    both adding into the same flat bucket (atomics) -- the sum equals the gradient of the whole batch in one pass.  (The schedule
    `bench.py --chains 2` measures; this pins that the library is safe to drive from two streams at once.  Under data parallelism the
    chains run with `dp.sync = False` -- a layer is only finished when BOTH halves have passed it -- and `finish()` ships the buckets.)"""
    dev = torch.device("cuda:0")
    from moka_amd.parallel import attach
    st, dims = _build("avt", dev)
    dp = attach(st, n_buckets=3)
    h, gout, mask_args, sl = _batch("avt", dims, dev)
    x_full = h.clone().requires_grad_(True)
    _run(st, dp, x_full, gout, mask_args, 1.0)
    dp.finish(average=False)
    torch.cuda.synchronize()
    ref, ref_dx = dp.bucket.flat.clone(), x_full.grad.clone()
    dp.bucket.flat.zero_()
    streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
    xs = [h[b:b + 1].clone().requires_grad_(True) for b in range(2)]
    torch.cuda.synchronize()
    with dp.no_sync():                                                # a layer is finished only when BOTH halves have passed it
        for b, sm in enumerate(streams):
            with torch.cuda.stream(sm):
                _run(st, dp, xs[b], gout[b:b + 1], sl(b, b + 1), 1.0)
    torch.cuda.synchronize()
    dp.finish(average=False)
    torch.cuda.synchronize()
    err = ((dp.bucket.flat - ref).norm() / ref.norm()).item()
    assert err <= 2e-4, err                                           # same products, another summation order
    for b in range(2):
        e = ((xs[b].grad.float() - ref_dx[b:b + 1].float()).norm() / ref_dx[b:b + 1].float().norm()).item()
        assert e <= 2e-2, (b, e)                                      # bf16 activations, per-sample vs batched launches


def test_sharded_frozen_base_under_the_real_stack_on_gpu():
    """SURVEY 8(f3) on hardware (world 1: the shard is the whole layer, the machinery is the same): the frozen tensors of every
    decoder layer live in ShardedFrozenBase, the layer hooks stage them into the two buffers for forward and backward, the
    adapter kernels read the staged base weight -- outputs and flat adapter gradients equal the plain stack's bit for bit."""
    dev = torch.device("cuda:0")
    from moka_amd.parallel import ShardedFrozenBase, attach
    st_a, dims = _build("avt", dev)
    st_b, _ = _build("avt", dev)
    h, gout, mask_args, _ = _batch("avt", dims, dev)
    dp_b = attach(st_b, n_buckets=3)
    _run(st_b, dp_b, h, gout, mask_args, 1.0)
    dp_b.finish()
    store = ShardedFrozenBase.shard_stack(st_a)
    assert all(p.numel() == 0 for n, p in st_a.named_parameters() if "lora_" not in n)
    dp_a = attach(st_a, n_buckets=3)
    with torch.no_grad():
        out_b, _ = st_b(h, *mask_args)
        out_a, _ = st_a(h, *mask_args)
    assert torch.equal(out_a, out_b)
    _run(st_a, dp_a, h, gout, mask_args, 1.0)
    dp_a.finish()
    torch.cuda.synchronize()
    err = ((dp_a.bucket.flat - dp_b.bucket.flat).norm() / dp_b.bucket.flat.norm()).item()
    assert err <= 1e-5, err                 # (atomics order only)
    assert store.shard_bytes() == sum(t.numel() * 2 for layer in st_b.layers for n, t in layer.named_parameters() if "lora_" not in n)


class _ProjectorThenStack(torch.nn.Module):
    """What both reference scripts train: a projector in front of the adapted decoder stack (finetune.py:151-160, train.py:573-579)."""

    def __init__(self, st, dims):
        super().__init__()
        torch.manual_seed(21)
        self.vl_projector = torch.nn.Linear(48, dims.hidden).to(next(st.parameters()).device, torch.bfloat16)
        self.model = st

    def forward(self, feats, *mask_args):
        return self.model(self.vl_projector(feats), *mask_args)


def _proj_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from moka_amd.parallel import attach
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    st, dims = _build("avt", dev)
    m = _ProjectorThenStack(st, dims)
    dp = attach(m, n_buckets=2)
    _, gout, _, sl = _batch("avt", dims, dev)
    feats = torch.randn(2, 96, 48, generator=torch.Generator().manual_seed(8)).to(dev, torch.bfloat16)
    out, _ = m(feats[rank:rank + 1], *sl(rank, rank + 1))
    (out.float() * gout[rank:rank + 1].float()).sum().backward()
    dp.finish(average=True)
    torch.cuda.synchronize()
    q.put((rank, dp.bucket.flat.cpu().numpy(), list(dp.names), list(dp.offsets), list(dp.hooked)))
    dist.barrier()
    dist.destroy_process_group()


def test_projector_in_front_of_the_stack_is_synchronised_with_the_adapter():
    """the non-adapter trainables ride in the same flat buffer and the same all-reduce.  Two ranks (one
    sample each, through the kernels) against ONE rank's mean gradient over both samples computed by plain autograd."""
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    st, dims = _build("avt", dev)
    m = _ProjectorThenStack(st, dims)
    h, gout, mask_args, _ = _batch("avt", dims, dev)
    feats = torch.randn(2, 96, 48, generator=torch.Generator().manual_seed(8)).to(dev, torch.bfloat16)
    out, _ = m(feats, *mask_args)
    (out.float() * gout.float()).sum().mul(0.5).backward()
    torch.cuda.synchronize()
    ref = {n: p.grad.float().cpu() for n, p in m.named_parameters() if p.grad is not None}
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_proj_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = [q.get(timeout=300) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
    import numpy as np
    assert (got[0][1] == got[1][1]).all(), "both ranks must hold the same averaged gradient"
    flat, names, offsets, hooked = torch.from_numpy(np.asarray(got[0][1])), got[0][2], got[0][3], got[0][4]
    assert set(hooked) == {"vl_projector.weight", "vl_projector.bias"}
    for n, o in zip(names, offsets):
        g = flat[o:o + ref[n].numel()].view_as(ref[n])
        err = ((g - ref[n]).norm() / ref[n].norm().clamp_min(1e-20)).item()
        assert err <= (2e-2 if n in hooked else 6e-3), (n, err)          # the reference went through bf16 autograd gradients


def test_bench_launches_its_own_ranks():
    """`python bench.py --gpus 2` with no launcher around it must BECOME two ranks (run as the driver runs it,
    it used to measure one GPU and print n_gpus 1).  Two gloo ranks share the one GPU: functional, never a measurement."""
    import json
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env["MOKA_BENCH_BACKEND"] = "gloo"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--layers", "2", "--steps", "2", "--warmup", "1",
                          "--full", "--no-cpu-baseline", "--no-traffic"], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["distributed"]["dist_world_size"] == 2 and out["distributed"]["backend"] == "gloo"
    assert out["value"] > 0 and abs(out["value"] - 2 * out["tokens_per_s_per_gpu"]) <= 1e-3 * out["value"]
    assert out["aggregate_tokens_per_s"] == out["value"] and out["comm_exposed_ms"] >= 0.0
    assert out["roofline"]["frac"] > 0 and "where" in out["roofline"]
    # asking for more ranks than devices over RCCL is a loud error, not a silent single-GPU run
    env["MOKA_BENCH_BACKEND"] = "nccl"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(torch.cuda.device_count() + 1), "--layers", "1",
                          "--steps", "1", "--no-cpu-baseline"], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert res.returncode != 0 and "GPU(s) visible" in (res.stderr + res.stdout)


@pytest.mark.parametrize("rank", [8, 40])
def test_deferred_dA_on_the_side_stream_gives_the_same_gradients(rank):
    """attach(defer_dA=True) (the default) launches the dA_m halves of a layer on a side stream when the layer's backward has been
    enqueued; the flat gradient must equal the in-chain schedule's (same kernels, same operands: only the atomics' order may differ),
    also with dropout (the mask is a function of (seed, token, column), not of the launch) and under gradient accumulation.
    rank 40 (rank pad 64): dB is a pass of its own there (moka_up_bwd_passes() == 2) and leaves the chain with dA_m."""
    dev = torch.device("cuda:0")
    from moka_amd import _lib
    from moka_amd.parallel import attach
    assert _lib.up_bwd_passes(8) == 1 and _lib.up_bwd_passes(32) == 1 and _lib.up_bwd_passes(40) == 2 and _lib.up_bwd_passes(8, _lib.MOKA_F32) == 2
    outs = []
    from moka_amd import functional as F
    batches, real = [], F.down_bwd_da_batch_

    def counted(dh_kmjs, xs, *a, **k):
        batches.append(len(xs))
        return real(dh_kmjs, xs, *a, **k)

    for defer in (False, True):
        st, dims = _build("avt", dev, rank=rank)
        for m in st.modules():
            if hasattr(m, "lora_dropout_p"):
                m.lora_dropout_p = 0.1
        dp = attach(st, n_buckets=3, defer_dA=defer)
        F.down_bwd_da_batch_ = counted
        h, gout, mask_args, sl = _batch("avt", dims, dev)
        torch.manual_seed(123)                                    # the dropout seeds are drawn from torch's CPU generator
        with dp.no_sync():
            _run(st, dp, h[:1], gout[:1], sl(0, 1), 1.0)
        _run(st, dp, h[1:], gout[1:], sl(1, 2), 1.0)
        assert (len(dp._deferred) == 0) or defer
        dp.finish(average=False)
        torch.cuda.synchronize()
        assert not dp._deferred and not dp._side_busy
        outs.append(dp.bucket.flat.clone())
        F.down_bwd_da_batch_ = real
        # a decoder layer's seven dA_m halves leave as ONE launch (moka_down_bwd_da_batch), two backward passes per run
        assert batches == ([7] * (2 * 3) if defer else []), batches          # (three layers)
        batches.clear()
    err = ((outs[0] - outs[1]).norm() / outs[0].norm()).item()
    assert outs[0].norm().item() > 0 and err <= 1e-5, err


def _opt_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from moka_amd.parallel import FlatAdamW, FlatGradBucket
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    n_layers, per = 6, 1024
    ends = [per * (l + 1) for l in range(n_layers)]
    bucket = FlatGradBucket(ends[-1], ends, dev, n_buckets=3)
    g = torch.Generator().manual_seed(3)
    master = torch.randn(ends[-1], generator=g).to(dev)
    work = torch.empty(ends[-1], device=dev, dtype=torch.bfloat16)
    opt = FlatAdamW(master, bucket.flat, work, lr=2e-3, betas=(0.9, 0.95), weight_decay=0.01)
    bucket.on_reduced = lambda lo, hi: opt.step_range(lo, hi, grad_scale=1.0 / world, zero_grad=True)
    for step in range(3):
        gr = torch.Generator().manual_seed(100 * step + rank)
        bucket.flat.copy_(torch.randn(ends[-1], generator=gr).to(dev))          # this rank's gradient
        opt.begin_step()
        for l in range(n_layers - 1, -1, -1):
            bucket.layer_done(l)          # a finished bucket: all-reduce on the communication stream, its AdamW slice right behind it
        bucket.finish(average=False)
        torch.cuda.synchronize()
    q.put((rank, master.cpu().numpy(), float(bucket.flat.abs().max())))
    dist.barrier()
    dist.destroy_process_group()


def test_optimizer_slices_behind_the_bucket_all_reduce_on_two_ranks():
    """FlatGradBucket.on_reduced: a bucket's AdamW update (FlatAdamW.step_range, coefficients in device memory) runs on the communication
    stream right behind its all-reduce; after three steps both ranks hold what one process gets from the averaged gradients in one launch."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_opt_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = {}
    for _ in range(2):
        r, m, gmax = q.get(timeout=240)
        got[r] = torch.from_numpy(m)
        assert gmax == 0.0
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    from moka_amd.parallel import FlatAdamW
    dev = torch.device("cuda:0")
    n = 6 * 1024
    master = torch.randn(n, generator=torch.Generator().manual_seed(3)).to(dev)
    grad, work = torch.zeros(n, device=dev), torch.empty(n, device=dev, dtype=torch.bfloat16)
    ref = FlatAdamW(master, grad, work, lr=2e-3, betas=(0.9, 0.95), weight_decay=0.01)
    for step in range(3):
        gs = sum(torch.randn(n, generator=torch.Generator().manual_seed(100 * step + r)) for r in range(2))
        grad.copy_(gs.to(dev))
        ref.step(grad_scale=0.5, zero_grad=True)
    torch.cuda.synchronize()
    assert torch.equal(got[0], got[1])
    err = ((got[0] - master.cpu()).norm() / master.cpu().norm()).item()
    assert err <= 1e-6, err


@pytest.mark.parametrize("defer", [True, False])
def test_optimizer_in_backward_takes_the_same_steps(defer):
    """attach(optimizer_in_backward=True): a finished bucket's AdamW slice runs on the side stream while the earlier layers' backward is
    still being enqueued; after three steps (the second one after a no_sync micro-batch) the parameters equal those of the step() that
    updates everything in one launch (same kernel arithmetic; the weight gradients' atomics may differ in order)."""
    dev = torch.device("cuda:0")
    from moka_amd.parallel import attach
    outs = []
    for inb in (False, True):
        st, dims = _build("avt", dev)
        dp = attach(st, n_buckets=3, lr=1e-2, weight_decay=0.01, defer_dA=defer, optimizer_in_backward=inb)
        h, gout, mask_args, sl = _batch("avt", dims, dev)
        for step in range(3):
            if step == 1:
                with dp.no_sync():
                    _run(st, dp, h[:1], gout[:1], sl(0, 1), 1.0)
                _run(st, dp, h[1:], gout[1:], sl(1, 2), 1.0)
            else:
                _run(st, dp, h, gout, mask_args, 0.5)
            dp.step()
        torch.cuda.synchronize()
        assert float(dp.bucket.flat.abs().max()) == 0.0 and dp.optimizer.t == 3
        outs.append((dp.master.clone(), dp.work.clone()))
    err = ((outs[0][0] - outs[1][0]).norm() / outs[0][0].norm()).item()
    assert err <= 1e-5, err
    assert (outs[0][1].float() - outs[1][1].float()).abs().max().item() <= 2 ** -6      # bf16 copies: at most an ulp of rounding apart
    # no clipping in this mode: said on EVERY call (one warning is lost in a training log), counted in state_dict(), and the
    # step neither throws behind the update nor changes anything
    with pytest.warns(RuntimeWarning, match="does NOT clip"):
        dp.step(max_grad_norm=1.0)
    with pytest.warns(RuntimeWarning, match="2 step"):
        dp.step(max_grad_norm=1.0)
    assert dp.state_dict()["unclipped_steps"] == 2 and dp.state_dict()["optimizer_in_backward"] is True
    torch.cuda.synchronize()


def _inb_worker(rank, world, port, inb, q):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from moka_amd.parallel import attach
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    st, dims = _build("avt", dev)
    dp = attach(st, n_buckets=2, lr=1e-2, optimizer_in_backward=inb)
    h, gout, _, sl = _batch("avt", dims, dev)
    for _ in range(2):
        _run(st, dp, h[rank:rank + 1], gout[rank:rank + 1], sl(rank, rank + 1), 1.0)
        dp.step()
    torch.cuda.synchronize()
    q.put((rank, dp.master.cpu().numpy()))
    dist.barrier()
    dist.destroy_process_group()


def test_optimizer_in_backward_on_two_ranks():
    """N > 1: the bucket's update runs on the communication stream behind its all-reduce (FlatGradBucket.on_reduced); both ranks end with the
    parameters the one-launch step gives."""
    ctx = mp.get_context("spawn")
    res = {}
    for inb in (False, True):
        q, port = ctx.Queue(), _free_port()
        procs = [ctx.Process(target=_inb_worker, args=(r, 2, port, inb, q)) for r in range(2)]
        for p in procs:
            p.start()
        got = dict(q.get(timeout=240) for _ in range(2))
        for p in procs:
            p.join(120)
            assert p.exitcode == 0
        assert (got[0] == got[1]).all()
        res[inb] = torch.from_numpy(got[0])
    err = ((res[True] - res[False]).norm() / res[False].norm()).item()
    assert err <= 1e-5, err


def _rccl_one_rank_worker(port, q):
    """One process, ONE-rank RCCL process group: the communication path of attach() as N > 1 ranks run it (ProcessGroupNCCL's own
    stream, in-place asynchronous all-reduce of a bucket slice, the bucket's AdamW slice on the communication stream behind it),
    against the short-circuit path, bit for bit (deterministic weight gradients; a one-rank sum is the identity)."""
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=dev)
    from moka_amd import functional as F
    from moka_amd.parallel import attach
    F.set_deterministic(True, device=dev)
    outs = []
    # (third run: bf16 payload -- the slice behind a bucket's all-reduce reads the bf16-rounded sum widened back into the fp32 buffer --
    #  and a tail bucket of one layer, the layout bench.py ships with)
    for force, cd, tail in ((False, None, None), (True, None, None), (True, torch.bfloat16, 1), (True, None, 1), (True, torch.bfloat16, None)):
        st, dims = _build("avt", dev)
        dp = attach(st, n_buckets=3, lr=1e-2, weight_decay=0.01, defer_dA=True, optimizer_in_backward=True, force_comm=force, comm_dtype=cd,
                    tail_layers=tail)
        assert dp.bucket.comm == force and dp.bucket.world == 1
        assert (dp.bucket.comm_stream is not None) == force
        if tail:
            assert len(dp.bucket.bucket_layers(0)) == 1
        assert dp.bucket.comm_dtype == cd
        h, gout, mask_args, sl = _batch("avt", dims, dev)
        for step in range(3):
            if step == 1:
                with dp.no_sync():
                    _run(st, dp, h[:1], gout[:1], sl(0, 1), 1.0)
                _run(st, dp, h[1:], gout[1:], sl(1, 2), 1.0)
            else:
                _run(st, dp, h, gout, mask_args, 0.5)
            if force:
                assert dp.bucket._pending, "no collective was issued"
            dp.step()
        torch.cuda.synchronize()
        assert float(dp.bucket.flat.abs().max()) == 0.0 and dp.optimizer.t == 3
        outs.append((dp.master.cpu().numpy(), dp.work.float().cpu().numpy()))
    backend = dist.get_backend()
    dist.destroy_process_group()
    q.put((backend, outs))


def test_one_rank_rccl_runs_the_communication_path_bit_for_bit():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_rccl_one_rank_worker, args=(_free_port(), q))
    p.start()
    backend, outs = q.get(timeout=100)
    p.join(120)
    assert p.exitcode == 0
    assert backend == "nccl"
    assert (outs[0][0] == outs[1][0]).all() and (outs[0][1] == outs[1][1]).all()
    # bf16 payload: every gradient element rounded to 8 bits once per step before AdamW (which normalises it): the three-step trajectories
    # agree to the rounding, and differ (the payload really was bf16)
    import numpy as np
    ref = outs[1][0]
    assert (outs[3][0] == ref).all()                       # the tail-bucket layout alone changes nothing (fp32 payload: bit for bit)
    for k in (2, 4):
        diff = outs[k][0] - ref
        rel = float(np.linalg.norm(diff) / np.linalg.norm(ref))
        assert 0.0 < rel <= 5e-3 and float(np.abs(diff).max()) <= 1.5e-2, (k, rel, float(np.abs(diff).max()))    # lr = 1e-2: at most ~one step's sign on a tiny gradient
    assert (outs[2][0] == outs[4][0]).all()                # (bf16 payload: the layout changes nothing either)


def test_bench_force_comm_prices_the_multi_gpu_configuration_on_one_gpu():
    """bench.py --force-comm: --graph bwd, the bucket hooks between the graphs and the AdamW slices behind each (one-rank RCCL) all-reduce."""
    import json
    import subprocess
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--force-comm", "--steps", "2", "--warmup", "1", "--layers", "4", "--batch", "1",
                          "--seq", "512", "--no-cpu-baseline", "--no-traffic"], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, (out.stdout[-1000:], out.stderr[-1000:])
    line = json.loads(lines[0])
    assert line["graph"] == "bwd" and line["distributed"]["backend"] == "nccl" and line["distributed"]["force_comm"] is True
    assert line["optimizer_in_backward"] is True and line["comm_exposed_ms"] >= 0.0 and line["value"] > 0


def test_lr_scheduler_drives_the_optimizer_inside_the_backward():
    """MokaFlatOptimizer on attach(optimizer_in_backward=True): the step's hyper-parameters are read from param_groups[0] when the step
    BEGINS (the first finished bucket of the backward), so the optimizer's own lr -- not the value attach() was given -- applies from
    the first step, and a scheduler's warm-up is not a step late; clipping is refused up front in this mode."""
    dev = torch.device("cuda:0")
    from moka_amd.parallel import MokaFlatOptimizer, attach
    outs = []
    for inb in (False, True):
        st, dims = _build("avt", dev)
        dp = attach(st, n_buckets=3, lr=1e-4, optimizer_in_backward=inb)          # (1e-4 must never be used)
        opt = MokaFlatOptimizer(dp, lr=2e-2, weight_decay=0.01)
        sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda k: [0.1, 0.5, 1.0, 1.0][min(k, 3)])
        h, gout, mask_args, _ = _batch("avt", dims, dev)
        lrs = []
        for _ in range(3):
            _run(st, dp, h, gout, mask_args, 0.5)
            opt.step()
            lrs.append(dp.optimizer.lr)
            sched.step()
        torch.cuda.synchronize()
        assert lrs == pytest.approx([2e-3, 1e-2, 2e-2]), lrs
        outs.append(dp.master.clone())
        if inb:
            with pytest.raises(ValueError):
                MokaFlatOptimizer(dp, max_grad_norm=1.0)
    err = ((outs[0] - outs[1]).norm() / outs[0].norm()).item()
    assert err <= 1e-5, err


def test_graphed_train_step_on_the_vt_mirror_equals_the_live_loop():
    """schedule.GraphedTrainStep around the VISUAL-TEXT mirror (modified_peft.Linear: two adapters, exact question index set, samples whose
    question spans differ): the captured step on two alternating batches == the live attach() loop, and the static routing is the one
    `from_vt_masks` compiles for every batch (the captured launches read it whatever masks the modules are handed)."""
    from moka_amd.parallel import attach
    from moka_amd.routing import MokaRouting
    from moka_amd.schedule import GraphedTrainStep
    dev = torch.device("cuda:0")

    def batches(dims):
        h, gout, (t, i, q), _ = _batch("vt", dims, dev)
        q2 = torch.zeros_like(q)
        q2[0, 50:55] = True
        q2[1, 62:80] = True
        return [{"h": h, "gout": gout, "t": t, "i": i, "q": q}, {"h": h.flip(0).contiguous(), "gout": gout, "t": t, "i": i, "q": q2}]

    def loss_of(st):
        return lambda p: (st(p["h"], p["t"], p["i"], p["q"])[0].float() * p["gout"].float()).sum() * (0.25 / p["h"].shape[0])

    st_r, dims = _build("vt", dev)
    bs = batches(dims)
    dp_r = attach(st_r, n_buckets=2, lr=1e-2, weight_decay=0.01)
    f_r, ref = loss_of(st_r), []
    for k in range(4):
        loss = f_r(bs[k % 2])
        loss.backward()
        dp_r.step()
        ref.append(float(loss.detach()))
    st, _ = _build("vt", dev)
    dp = attach(st, n_buckets=2, lr=1e-2, weight_decay=0.01)
    gs = GraphedTrainStep(dp, loss_of(st), bs[0], routing_fn=lambda p: MokaRouting.from_vt_masks(p["t"], p["i"], p["q"]))
    got = [float(gs(bs[k % 2])) for k in range(4)]
    torch.cuda.synchronize()
    assert got[0] == ref[0]                                       # the same kernels on the same data before any update
    for a_, b_ in zip(got, ref):
        assert abs(a_ - b_) <= 2e-3 * abs(b_) + 1e-6, (got, ref)
    err = ((dp.master - dp_r.master).norm() / dp_r.master.norm()).item()
    assert err <= 2e-4, err
    assert gs.rts[0].klen.tolist() == MokaRouting.from_vt_masks(bs[1]["t"], bs[1]["i"], bs[1]["q"]).klen.tolist()     # the last batch's routing sits in the static buffers


def _graph_rank(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from moka_amd.parallel import attach
    from moka_amd.routing import MokaRouting
    from moka_amd.schedule import GraphedTrainStep
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    h, gout, (masks,), sl = None, None, (None,), None
    outs = []
    for graphed in (False, True):
        st, dims = _build("avt", dev)
        dp = attach(st, n_buckets=2, lr=1e-2, weight_decay=0.01)
        h, gout, (masks,), sl = _batch("avt", dims, dev)
        if not graphed:                                        # the live loop of the same rank: bucketed all-reduce behind the backward, one fused AdamW
            for _ in range(3):
                _run(st, dp, h[rank:rank + 1], gout[rank:rank + 1], sl(rank, rank + 1), 0.5)
                dp.step()
        else:
            mine = {"h": h[rank:rank + 1], "gout": gout[rank:rank + 1], **{"m%d" % k: m[rank:rank + 1] for k, m in enumerate(masks)}}
            gs = GraphedTrainStep(dp, lambda p: (st(p["h"], [p["m0"], p["m1"], p["m2"], p["m3"]])[0].float() * p["gout"].float()).sum() * 0.5, mine,
                                  routing_fn=lambda p: MokaRouting.from_avt_masks([p["m0"], p["m1"], p["m2"], p["m3"]]))
            assert gs.opt_in_graph is False and len(gs.capture_log) == 1
            for _ in range(3):
                gs(mine)
        torch.cuda.synchronize()
        outs.append((dp.master.cpu().numpy(), dp.optimizer.t))
    q.put((rank, outs))
    dist.barrier()
    dist.destroy_process_group()


def test_graphed_train_step_under_two_ranks_sums_the_gradient_behind_the_replay():
    """GraphedTrainStep with collectives on (two gloo ranks on the one GPU, one sample each): RCCL cannot ride inside a capture, so the graph ends
    with the local gradient and ONE all-reduce of the flat buffer + the fused AdamW follow it live; both ranks end with the same parameters, and
    those are the parameters of the LIVE attach() loop of the same two ranks (bucketed all-reduce behind the backward)."""
    ctx = mp.get_context("spawn")
    q, port = ctx.Queue(), _free_port()
    procs = [ctx.Process(target=_graph_rank, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=300) for _ in range(2))
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    (live0, t_l), (graph0, t_g) = got[0]
    (live1, _), (graph1, _) = got[1]
    assert t_l == t_g == 3 and (graph0 == graph1).all() and (live0 == live1).all()
    a_, b_ = torch.from_numpy(graph0), torch.from_numpy(live0)
    err = ((a_ - b_).norm() / b_.norm()).item()
    assert err <= 1e-5, err                                    # the same arithmetic: only the order of the fp32 atomics differs
