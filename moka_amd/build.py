"""In-tree build of libmoka_hip.so for gfx950 (hipcc cross-compiles without a GPU).

    python -m moka_amd.build [--force] [--unity]

and of libmoka_decode.so, the decode-step kernel (csrc/moka_decode.hip, one translation unit), and libmoka_dlinear.so, the decode-step
projection with the base GEMV inside (csrc/moka_dlinear.hip, one translation unit), beside it; the two share csrc/moka_step.h.

The library is six translation units (moka_amd/csrc/k_*.hip: one per kernel family, moka_api.hip: the entry points and launch rules)
compiled in parallel and linked; a change to the launch rules rebuilds in seconds, a change to one kernel family rebuilds that family.
``--unity`` compiles csrc/moka_kernels.hip (all of them in one) instead.  The .so is git-ignored but travels to the GPU box with the
gpurun snapshot; the object files under csrc/_obj/ are a local cache.
"""
from __future__ import annotations

import concurrent.futures
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
UNITS = ["k_cross", "k_expand", "k_wgrad", "k_reduce", "k_misc", "moka_api"]
HEADERS = [os.path.join(CSRC, "moka_device.h"), os.path.join(CSRC, "moka_host.h"), os.path.join(ROOT, "include", "moka_hip.h")]
SRC = os.path.join(CSRC, "moka_kernels.hip")               # the unity form (tools/microbench/passlab.hip, tools/kernel_resources.sh)
OUT = os.path.join(HERE, "libmoka_hip.so")
DECODE_SRC = os.path.join(CSRC, "moka_decode.hip")         # the decode-step kernel: a library of its own (include/moka_decode.h)
OUT_DECODE = os.path.join(HERE, "libmoka_decode.so")
DLINEAR_SRC = os.path.join(CSRC, "moka_dlinear.hip")       # base GEMV + adapter in one launch: a library of its own (include/moka_dlinear.h)
OUT_DLINEAR = os.path.join(HERE, "libmoka_dlinear.so")
STEP_HDR = os.path.join(CSRC, "moka_step.h")               # what the two decode-step kernels share; no part of libmoka_hip.so
INC = os.path.join(ROOT, "include")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-Wno-unused-function", "-munsafe-fp-atomics", "-I", INC, "-I", CSRC]


def sources():
    """Every file the library is built from (what a PMC traffic summary is stamped with: bench.kernel_source_sha256)."""
    return [os.path.join(CSRC, u + ".hip") for u in UNITS] + HEADERS


def _hipcc() -> str:
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (expected /opt/rocm/bin/hipcc)")


def needs_build(out: str = OUT) -> bool:
    if not os.path.exists(out):
        return True
    return os.path.getmtime(out) < max(os.path.getmtime(p) for p in sources())


def _run(cmd, verbose, what="libmoka_hip.so"):
    if verbose:
        print(" ".join(cmd), flush=True)
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        sys.stderr.write(res.stdout + res.stderr)
        raise RuntimeError("hipcc failed building " + what)


def decode_sources():
    """Every file libmoka_decode.so is built from.  Kept apart from ``sources()``: that list is what the traffic summaries of
    libmoka_hip.so are stamped with, and the decode kernel is no part of that library."""
    return [DECODE_SRC, STEP_HDR, os.path.join(ROOT, "include", "moka_decode.h")] + HEADERS


def dlinear_sources():
    """Every file libmoka_dlinear.so is built from (kept apart from ``sources()`` and ``decode_sources()`` for the same reason)."""
    return [DLINEAR_SRC, STEP_HDR, os.path.join(ROOT, "include", "moka_dlinear.h")] + HEADERS


def _build_one(src: str, out: str, srcs, label: str, force: bool, verbose: bool) -> str:
    """A library of one translation unit, compiled and linked in one go unless it is newer than everything it is built from."""
    if not force and os.path.exists(out) and os.path.getmtime(out) >= max(os.path.getmtime(p) for p in srcs):
        return out
    _run([_hipcc()] + FLAGS + ["-shared", src, "-o", out + ".tmp"], verbose, label)
    os.replace(out + ".tmp", out)
    return out


def build_decode(force: bool = False, verbose: bool = True) -> str:
    """libmoka_decode.so (include/moka_decode.h): the decode-step adapter kernel."""
    return _build_one(DECODE_SRC, OUT_DECODE, decode_sources(), "libmoka_decode.so", force, verbose)


def build_dlinear(force: bool = False, verbose: bool = True) -> str:
    """libmoka_dlinear.so (include/moka_dlinear.h): the decode-step projection, base GEMV and adapter in one launch."""
    return _build_one(DLINEAR_SRC, OUT_DLINEAR, dlinear_sources(), "libmoka_dlinear.so", force, verbose)


def build(force: bool = False, verbose: bool = True, unity: bool = False) -> str:
    """Also brings libmoka_decode.so and libmoka_dlinear.so up to date (``build_decode``, ``build_dlinear``); the path returned is
    libmoka_hip.so's."""
    out = OUT
    build_decode(force=force, verbose=verbose)
    build_dlinear(force=force, verbose=verbose)
    if not force and not needs_build(out):
        return out
    cc = _hipcc()
    if unity:
        _run([cc] + FLAGS + ["-shared", SRC, "-o", out + ".tmp"], verbose)
        os.replace(out + ".tmp", out)
        return out
    objdir = os.path.join(CSRC, "_obj")
    os.makedirs(objdir, exist_ok=True)
    newest_hdr = max(os.path.getmtime(h) for h in HEADERS)
    jobs = []
    for u in UNITS:
        src, obj = os.path.join(CSRC, u + ".hip"), os.path.join(objdir, u + ".o")
        if force or not os.path.exists(obj) or os.path.getmtime(obj) < max(os.path.getmtime(src), newest_hdr):
            jobs.append([cc] + FLAGS + ["-c", src, "-o", obj])
    with concurrent.futures.ThreadPoolExecutor(max_workers=max(1, min(len(jobs) or 1, os.cpu_count() or 1))) as ex:
        list(ex.map(lambda c: _run(c, verbose), jobs))
    _run([cc, "--offload-arch=gfx950", "-shared", "-fPIC"] + [os.path.join(objdir, u + ".o") for u in UNITS] + ["-o", out + ".tmp"], verbose)
    os.replace(out + ".tmp", out)
    return out


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, unity="--unity" in sys.argv))
