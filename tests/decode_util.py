"""What the tests of the two decode-step libraries share (tests/test_gpu_decode.py, tests/test_gpu_dlinear.py, tests/test_decode_host.py,
tests/test_dlinear_host.py): the error measures, the raw entry-point calls, the PEFT mirror modules and the decoder stack they go
through, and the header / ctypes helpers of the host tests.  A plain module: no fixtures, no tests."""
import ctypes
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16


# ------------------------------------------------------------------------------------------ host tests
def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(moka_[a-z_0-9]+)\s*\(", src)))


def _ints(vals):
    return (ctypes.c_int * len(vals))(*vals)


# ------------------------------------------------------------------------------------------ measures
def _dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    n = b.norm().item()
    d = (a - b).norm().item()
    return d / n if n > 0 else d


def ulp_bf16_diff(a_bf16, b_bf16, operand=None):
    """max |a - b| in bf16 ulps, the measure of tests/test_gpu_parity.py::_stage_check: the ulp is taken at max(|b|, |operand|) (the kernel
    computes operand + delta), elements below rms / 256 are measured at that floor (the hi + lo split carries 2^-17 of each TERM)."""
    a, b = a_bf16.float().cpu(), b_bf16.float().cpu()
    mag = b.abs() if operand is None else torch.maximum(b.abs(), operand.float().cpu().abs().reshape(b.shape))
    mag = mag.clamp_min(float(b.pow(2).mean().sqrt()) / 256)
    ulp = torch.pow(2.0, torch.floor(torch.log2(mag.clamp_min(1e-30))) - 7)
    return ((a - b).abs() / ulp).max().item()


# ------------------------------------------------------------------------------------------ the entry points on raw tensors
def _arr(tensors):
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def decode_fwd(x, As, Bs, ys, r, scale):
    """moka_decode_fwd on raw tensors (x [T, d_in], A_g [r, d_in], B_g [d_out_g, r], y_g [T, d_out_g], in place on ys)."""
    from moka_amd import _decode_lib
    lib = _decode_lib.load()
    T, d_in = x.shape
    d_outs = (ctypes.c_int * len(ys))(*[y.shape[1] for y in ys])
    rc = lib.moka_decode_fwd(x.data_ptr(), _arr(As), _arr(Bs), _arr(ys), d_outs, len(ys), T, d_in, r, float(scale),
                             ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream))
    assert rc == 0, _decode_lib.last_error()


def dlinear_fwd(x, Ws, biases, As, Bs, ys, r, scale, T=None):
    """moka_dlinear_fwd on raw tensors (x [T, d_in], W_g [d_out_g, d_in], bias_g [d_out_g] | None, A_g [r, d_in], B_g [d_out_g, r],
    y_g [>= T, d_out_g] written)."""
    from moka_amd import _dlinear_lib
    lib = _dlinear_lib.load()
    d_in = x.shape[1]
    T = x.shape[0] if T is None else T
    d_outs = (ctypes.c_int * len(ys))(*[y.shape[1] for y in ys])
    barr = None if biases is None or all(b is None for b in biases) else _arr(biases)
    rc = lib.moka_dlinear_fwd(x.data_ptr(), _arr(Ws), barr, _arr(As), _arr(Bs), _arr(ys), d_outs, len(ys), T, d_in, r, float(scale),
                              ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream))
    assert rc == 0, _dlinear_lib.last_error()


# ------------------------------------------------------------------------------------------ the PEFT mirrors
def _avt_module(cd, dev, zero_base=False, p=0.0):
    from moka_amd.peft_hyper import Linear
    c = cd.case
    lin = Linear(c.d_in, c.d_out, r=(c.r,) * 3, lora_alpha=c.alpha, lora_nums=3, blc_weight=c.w, blc_alpha=1, lora_dropout=p,
                 loramethod="test", bias=False).to(dev, BF)
    with torch.no_grad():
        lin.weight.copy_(torch.zeros_like(cd.W) if zero_base else cd.W)
        for i in range(len(cd.A)):
            getattr(lin, f"lora_A{i}").weight.copy_(cd.A[i])
        lin.lora_B0.weight.copy_(cd.Bw)
    return lin


def _vt_module(cd, dev, zero_base=False, p=0.0, bias=False):
    from moka_amd.modified_peft import Linear as VtLinear
    c = cd.case
    base = torch.nn.Linear(c.d_in, c.d_out, bias=bias)
    base.weight.requires_grad_(False)                           # the frozen base
    if bias:
        base.bias.requires_grad_(False)
    m = VtLinear(base, "image", r=c.r, lora_alpha=c.alpha, lora_dropout=p, attn_weight=c.w)
    m.update_layer("text", c.r, lora_alpha=c.alpha, lora_dropout=p, init_lora_weights=True, use_rslora=False)
    m.set_adapter(["image", "text"])
    m = m.to(dev, BF)
    with torch.no_grad():
        m.get_base_layer().weight.copy_(torch.zeros_like(cd.W) if zero_base else cd.W)
        m.lora_A["text"].weight.copy_(cd.A[0])
        m.lora_B["text"].weight.copy_(cd.Bw)
        if len(cd.A) > 1:
            m.lora_A["image"].weight.copy_(cd.A[1])
    return m


def _mirror_call(kind, mod, x):
    return mod(x, None) if kind == "avt" else mod(x, None, None, None)


# ------------------------------------------------------------------------------------------ the decoder
def _stack(dev, r=16, n_layers=2):
    from moka_amd.decoder import LlamaDims, MokaLlamaStack
    from moka_amd.peft_hyper import Linear
    dims = LlamaDims(hidden=128, ff=352, n_heads=4, n_kv_heads=2)           # the DIMS of tests/test_decoder_layer.py
    torch.manual_seed(1)

    def make(d_in, d_out):
        m = Linear(d_in, d_out, r=(r, r, r), lora_alpha=16, lora_nums=3, blc_weight=1.0, blc_alpha=1, lora_dropout=0.0,
                   loramethod="test", bias=False)
        torch.nn.init.normal_(m.lora_B0.weight, std=0.05)
        return m

    return MokaLlamaStack(dims, n_layers, make).to(dev, BF).eval(), dims


def _avt_masks(B, S, dev):
    """[text, video, audio, question] int32 [B, S, 1]: 8 text, 24 video, 8 text, 16 audio, 12 question, rest text."""
    tok = torch.zeros(S, dtype=torch.long)
    tok[8:32] = 1
    tok[40:56] = 2
    q = torch.zeros(S, dtype=torch.int32)
    q[56:68] = 1
    ms = [(tok == m).to(torch.int32).reshape(1, S, 1).repeat(B, 1, 1).to(dev) for m in range(3)]
    return ms + [q.reshape(1, S, 1).repeat(B, 1, 1).to(dev)]
