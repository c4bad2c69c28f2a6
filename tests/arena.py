"""Guard-banded buffers for the buffer-contract tests (a helper module, not a conftest).

An ``Arena`` places every caller-owned buffer of one entry-point call as a contiguous view inside ONE allocation, each with a guard
band before and after it, so that a stray access of a tail tile or a split-K chunk stays inside the allocation and is observed
(never faults).  What it checks after the call (``check()``):

  * the guards are bit-identical: nothing was written past the end or before the start of a buffer;
  * the inputs are bit-identical: no kernel writes what it reads;
  * ``write`` buffers (poisoned with NaN before the call) hold no NaN anywhere in their documented extent (``exempt``: elements
    the contract leaves unspecified), and their documented padding (``zero``) is exactly zero;
  * ``inout`` buffers (seeded finite values before the call) are returned as ``after - before`` by ``delta()``.

Guards around inputs hold NaN, so that a stray READ that reaches a result shows up there; guards around outputs hold a fixed
seeded byte pattern.  ``shift`` places every buffer that many bytes past a 256-byte boundary (0: the default placement; 16-byte
aligned shifts test the pointers the header promises no alignment for).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional

import torch

ROLES = ("input", "write", "inout", "workspace")
ALIGN = 256
MIN_GUARD = 1 << 20
_NAN_BITS = {torch.bfloat16: (0x7FC0, torch.int16), torch.float32: (0x7FC00000, torch.int32)}
_POISON_INT = 0xA5                      # `write` buffers of an integer type: a byte no kernel output of this project holds


@dataclass
class Buf:
    shape: tuple
    dtype: torch.dtype
    role: str
    data: Optional[torch.Tensor] = None     # input / inout: the values before the call
    zero: Optional[torch.Tensor] = None     # write: bool mask of the documented padding (must be exactly zero)
    exempt: Optional[torch.Tensor] = None   # write: bool mask of elements the contract leaves unspecified
    fill: str = "garbage"                   # workspace: "garbage" (seeded random bits), "nan" or "zero"
    flat: bool = False                      # no token / weight rows (operand pack planes): does not size the guards

    def __post_init__(self):
        assert self.role in ROLES, self.role
        self.shape = tuple(int(s) for s in self.shape)
        if self.role in ("input", "inout"):
            assert self.data is not None and tuple(self.data.shape) == self.shape, "input / inout buffers need data of their shape"

    @property
    def numel(self):
        n = 1
        for s in self.shape:
            n *= s
        return n

    @property
    def esize(self):
        return torch.empty((), dtype=self.dtype).element_size()

    @property
    def nbytes(self):
        return self.numel * self.esize

    @property
    def row_bytes(self):
        """Bytes of one token / weight row: the last dimension of a 2-D buffer (1-D workspaces and buffers marked `flat` have no rows)."""
        return self.shape[-1] * self.esize if len(self.shape) == 2 and not self.flat else 0


def _align(n, a=ALIGN):
    return (n + a - 1) // a * a


def guard_bytes(bufs) -> int:
    """At least 1 MiB, and at least one 128-token block of the widest row plus one 512-column chunk of the widest element."""
    rows = max((b.row_bytes for b in bufs), default=0)
    es = max((b.esize for b in bufs), default=4)
    return _align(max(MIN_GUARD, 128 * rows + 512 * es))


class ContractError(AssertionError):
    pass


class Arena:
    def __init__(self, device, spec: Dict[str, Buf], shift: int = 0, seed: int = 0):
        assert shift % 16 == 0 and 0 <= shift < ALIGN, "shift: a multiple of 16 below 256"
        self.device = torch.device(device)
        self.spec = dict(spec)
        self.shift = shift
        bufs = list(self.spec.values())
        self.guard = guard_bytes(bufs)
        # layout: [guard][buffer][guard] per buffer; the buffer starts `shift` bytes past a 256-byte boundary, the guard before it
        # covers everything from the end of the previous band, the guard after it starts at its last byte + 1
        self.place = {}
        cur = 0
        for name, b in self.spec.items():
            g0 = cur
            start = _align(cur + self.guard) + shift
            end = start + b.nbytes
            self.place[name] = (g0, start, end, end + self.guard)
            cur = end + self.guard
        total = _align(cur)
        self.mem = torch.empty(total, dtype=torch.uint8, device=self.device)
        gen = torch.Generator(device=self.device).manual_seed(0x5EED + seed)
        rnd = lambda n: torch.randint(0, 256, (n,), generator=gen, dtype=torch.uint8, device=self.device)   # noqa: E731
        for name, b in self.spec.items():
            g0, start, end, g1 = self.place[name]
            for lo, hi in ((g0, start), (end, g1)):
                if b.role == "input":
                    self._fill_nan(lo, hi, b.dtype)
                else:
                    self.mem[lo:hi] = rnd(hi - lo)
            v = self.view(name)
            if b.role in ("input", "inout"):
                v.copy_(b.data.to(self.device, b.dtype).reshape(b.shape))
            elif b.role == "write":
                self._poison(name)
            elif b.fill == "zero":
                self.mem[start:end] = 0
            elif b.fill == "nan":
                self._fill_nan(start, end, b.dtype if b.dtype in _NAN_BITS else torch.float32)
            else:
                self.mem[start:end] = rnd(end - start)
        self.before = self.mem.clone()

    # ---- placement
    def view(self, name) -> torch.Tensor:
        b = self.spec[name]
        _, start, end, _ = self.place[name]
        return self.mem[start:end].view(b.dtype).view(b.shape)

    def ptr(self, name) -> int:
        return self.view(name).data_ptr()

    def prior(self, name) -> torch.Tensor:
        b = self.spec[name]
        _, start, end, _ = self.place[name]
        return self.before[start:end].view(b.dtype).view(b.shape)

    def delta(self, name) -> torch.Tensor:
        """after - before of an inout buffer, in fp64."""
        assert self.spec[name].role == "inout"
        return self.view(name).double() - self.prior(name).double()

    def check_delta(self, name, expected, tol, mask=None) -> float:
        """Relative Frobenius error of delta(name) against `expected` (fp64; optionally over `mask` only); a ContractError beyond
        `tol`.  With a prior of the delta's own magnitude, an accumulator a kernel overwrote instead of adding to is off by ~1."""
        d = self.delta(name).cpu()
        e = expected.double().cpu().reshape(d.shape)
        if mask is not None:
            d, e = d[mask], e[mask]
        n = e.norm().item()
        err = (d - e).norm().item() / (n if n > 0 else 1.0)
        if not err <= tol:
            raise ContractError(f"{name}: after - before is {err:.3g} away from the expected increment (tolerance {tol:g})")
        return err

    # ---- fills
    def _fill_nan(self, lo, hi, dtype):
        if dtype not in _NAN_BITS:
            self.mem[lo:hi] = 0xFF
            return
        bits, idt = _NAN_BITS[dtype]
        es = torch.empty((), dtype=dtype).element_size()
        a0, a1 = _align(lo, es), hi // es * es
        self.mem[lo:a0] = 0xFF
        self.mem[a1:hi] = 0xFF
        if a1 > a0:
            w = self.mem[a0:a1].view(idt)
            w.fill_(bits if bits < (1 << (8 * es - 1)) else bits - (1 << (8 * es)))

    def _poison(self, name):
        b = self.spec[name]
        _, start, end, _ = self.place[name]
        if b.dtype.is_floating_point:
            self._fill_nan(start, end, b.dtype)
        else:
            self.mem[start:end] = _POISON_INT

    # ---- checks
    def guard_damage(self):
        """[(buffer, side, first, last)]: element offsets (in the buffer's element size) of the changed guard bytes -- `after`: counted
        from the buffer's end (0 = the first element past it), `before`: counted backwards from its start (0 = the element just before)."""
        out = []
        for name, b in self.spec.items():
            g0, start, end, g1 = self.place[name]
            for side, lo, hi in (("before", g0, start), ("after", end, g1)):
                if torch.equal(self.mem[lo:hi], self.before[lo:hi]):
                    continue
                idx = torch.nonzero(self.mem[lo:hi] != self.before[lo:hi]).flatten().cpu()
                a, z = int(idx[0]) + lo, int(idx[-1]) + lo
                if side == "after":
                    out.append((name, side, (a - end) // b.esize, (z - end) // b.esize))
                else:
                    out.append((name, side, (start - 1 - z) // b.esize, (start - 1 - a) // b.esize))
        return out

    def problems(self):
        msgs = []
        for name, side, a, z in self.guard_damage():
            where = "past the end" if side == "after" else "before the start"
            msgs.append(f"{name}: written {where} (elements {a}..{z} {where})")
        for name, b in self.spec.items():
            v = self.view(name)
            _, start, end, _ = self.place[name]
            if b.role == "input":
                if not torch.equal(self.mem[start:end], self.before[start:end]):
                    n = int((self.mem[start:end] != self.before[start:end]).sum())
                    msgs.append(f"{name}: input modified ({n} bytes changed)")
            elif b.role == "write":
                bad = torch.isnan(v) if b.dtype.is_floating_point else (v == _POISON_INT)
                if b.exempt is not None:
                    bad = bad & ~b.exempt.to(self.device).reshape(b.shape)
                if bool(bad.any()):
                    first = torch.nonzero(bad)[0].tolist()
                    msgs.append(f"{name}: {int(bad.sum())} element(s) never written (first at {first})")
                if b.zero is not None:
                    z = b.zero.to(self.device).reshape(b.shape)
                    nz = z & (v != 0)
                    if bool(nz.any()):
                        first = torch.nonzero(nz)[0].tolist()
                        msgs.append(f"{name}: {int(nz.sum())} padding element(s) not zero (first at {first})")
        return msgs

    def check(self):
        msgs = self.problems()
        if msgs:
            raise ContractError("; ".join(msgs))
