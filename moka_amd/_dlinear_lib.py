"""ctypes binding of libmoka_dlinear.so (the C ABI declared in include/moka_dlinear.h): the decode-step projection, base GEMV with the
adapter fused.

A library of its own beside libmoka_hip.so (``_lib``) and libmoka_decode.so (``_decode_lib``), built by the same
``__graft_entry__.build()`` / ``python -m moka_amd.build``.  As there, NO fallback: a missing shared object raises ``MokaError``.
"""
from __future__ import annotations

import os
from ctypes import POINTER, c_char_p, c_float, c_int, c_void_p

from ._lib import MOKA_BF16, MOKA_F32, MokaError, open_library   # noqa: F401  (the dtype codes are those of include/moka_hip.h)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmoka_dlinear.so")

_lib = None

# name -> (restype, argtypes); must list EVERY symbol include/moka_dlinear.h declares
SYMBOLS = {
    "moka_dlinear_version": (c_int, []),
    "moka_dlinear_last_error": (c_char_p, []),
    "moka_dlinear_max_tokens": (c_int, []),
    # T, d_in, d_out[G], G, r, dtype
    "moka_dlinear_ok": (c_int, [c_int, c_int, POINTER(c_int), c_int, c_int, c_int]),
    # x, W[G], bias[G] | NULL, A[G], Bw[G], y_out[G], d_out[G], G, T, d_in, r, scale, stream
    "moka_dlinear_fwd": (c_int, [c_void_p, POINTER(c_void_p), POINTER(c_void_p), POINTER(c_void_p), POINTER(c_void_p), POINTER(c_void_p),
                                 POINTER(c_int), c_int, c_int, c_int, c_int, c_float, c_void_p]),
    # d_out[G], G, d_in, r
    "moka_dlinear_workgroups": (c_int, [POINTER(c_int), c_int, c_int, c_int]),
}


def load():
    """Load the shared library (once).  Raises MokaError when it has not been built."""
    global _lib
    if _lib is None:
        _lib = open_library(LIB_PATH, SYMBOLS, "the decode-step projection HIP library")
    return _lib


def last_error() -> str:
    return load().moka_dlinear_last_error().decode("utf-8", "replace")


def check(rc: int, what: str = ""):
    if rc != 0:
        raise MokaError(f"{what or 'moka_dlinear'} failed with code {rc}: {last_error()}")


def dlinear_ok(T: int, d_in: int, d_outs, r: int, dtype: int = MOKA_BF16) -> bool:
    """True when moka_dlinear_fwd takes the call.  Arguments no path accepts come back as False too -- the paths below it then raise
    their own error for them."""
    d = [int(v) for v in d_outs]
    return load().moka_dlinear_ok(int(T), int(d_in), (c_int * len(d))(*d), len(d), int(r), int(dtype)) == 1
