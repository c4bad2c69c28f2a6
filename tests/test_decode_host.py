"""CPU: the decode-step library (include/moka_decode.h) builds for gfx950 beside libmoka_hip.so without entering it, exports what its
header declares, validates its arguments on the host, and the Python dispatch rule sends it exactly the calls it is meant for."""
import ctypes
import os

import pytest
import torch

from tests.decode_util import ROOT, _declared, _ints

BF16, F32 = 0, 1


@pytest.fixture(scope="module")
def libs():
    from moka_amd import _decode_lib, _lib, build
    path = build.build(verbose=False)          # hipcc cross-compiles without a GPU; no-op when up to date
    assert os.path.basename(path) == "libmoka_hip.so"
    return _lib.load(), _decode_lib.load()


def test_build_produces_both_libraries(libs):
    from moka_amd import _decode_lib, build
    assert os.path.exists(build.OUT) and os.path.exists(build.OUT_DECODE)
    assert _decode_lib.LIB_PATH == build.OUT_DECODE
    assert build.build_decode(verbose=False) == build.OUT_DECODE          # up to date: a no-op
    assert libs[1].moka_decode_version() >= 100
    assert libs[1].moka_decode_max_tokens() == 64


def test_every_declared_symbol_is_exported_and_bound(libs):
    from moka_amd import _decode_lib
    declared = _declared("moka_decode.h")
    assert len(declared) == 5 and all(n.startswith("moka_decode_") for n in declared)
    for name in declared:
        assert hasattr(libs[1], name), f"{name} declared in moka_decode.h but not exported"
    assert sorted(_decode_lib.SYMBOLS) == declared


def test_the_training_library_holds_nothing_of_it(libs):
    from moka_amd import _lib
    assert not [n for n in _declared("moka_hip.h") if n.startswith("moka_decode")]
    assert not [n for n in _lib.SYMBOLS if n.startswith("moka_decode")]
    for name in _declared("moka_decode.h"):
        assert not hasattr(libs[0], name), f"libmoka_hip.so exports {name}"


def test_the_pinned_source_list_is_unchanged():
    from moka_amd import _decode_lib, build
    assert _decode_lib.LIB_PATH == build.OUT_DECODE != build.OUT
    assert not set(build.sources()) & {build.DECODE_SRC, os.path.join(ROOT, "include", "moka_decode.h")}
    assert build.UNITS == ["k_cross", "k_expand", "k_wgrad", "k_reduce", "k_misc", "moka_api"]
    assert [os.path.basename(h) for h in build.HEADERS] == ["moka_device.h", "moka_host.h", "moka_hip.h"]
    names = [os.path.basename(p) for p in build.sources()]
    assert names == [u + ".hip" for u in build.UNITS] + ["moka_device.h", "moka_host.h", "moka_hip.h"]
    assert not [n for n in names if "decode" in n]
    unity = open(build.SRC).read()
    assert "moka_decode" not in unity


def test_decode_ok_table(libs):
    ok = libs[1].moka_decode_ok
    one = _ints([4096])
    assert [ok(T, 4096, one, 1, 16, BF16) for T in (1, 64)] == [1, 1]
    assert [ok(T, 4096, one, 1, 16, BF16) for T in (0, 65)] == [0, 0]            # valid shapes of the general path
    assert [ok(4, 4096, one, 1, r, BF16) for r in (1, 16, 17, 64)] == [1, 1, 1, 1]
    assert all(ok(4, 4096, one, 1, r, BF16) < 0 for r in (0, 65))
    assert ok(4, 4096, one, 0, 16, BF16) < 0 and ok(4, 4096, _ints([64] * 4), 4, 16, BF16) < 0
    assert ok(4, 4096, _ints([256, 64, 64]), 3, 16, BF16) == 1
    assert ok(4, 72, one, 1, 16, BF16) < 0 and ok(4, 4096, _ints([72]), 1, 16, BF16) < 0
    assert b"multiple of 32" in libs[1].moka_decode_last_error()
    assert ok(4, 4096, _ints([64, 72]), 2, 16, BF16) < 0
    assert ok(4, 4096, None, 1, 16, BF16) < 0
    assert ok(4, 4096, one, 1, 16, F32) == 0
    assert ok(4, 4096, one, 1, 16, 7) < 0


def test_decode_fwd_validates_on_the_host(libs):
    """Every refusal comes back before a launch (this test runs without a device): fake, aligned, non-null addresses are never touched."""
    fwd, err = libs[1].moka_decode_fwd, libs[1].moka_decode_last_error
    p = ctypes.c_void_p(0x10000)
    arr = (ctypes.c_void_p * 1)(0x10000)
    null1 = (ctypes.c_void_p * 1)(None)
    d = _ints([64])
    assert fwd(None, arr, arr, arr, d, 1, 4, 64, 16, 1.0, None) < 0 and b"null" in err()
    assert fwd(p, None, arr, arr, d, 1, 4, 64, 16, 1.0, None) < 0 and b"null" in err()
    assert fwd(p, arr, arr, null1, d, 1, 4, 64, 16, 1.0, None) < 0 and b"null" in err()
    assert fwd(p, arr, arr, arr, None, 1, 4, 64, 16, 1.0, None) < 0 and b"null" in err()
    assert fwd(p, arr, arr, arr, d, 1, 4, 72, 16, 1.0, None) < 0 and b"multiple of 32" in err()
    assert fwd(p, arr, arr, arr, _ints([72]), 1, 4, 64, 16, 1.0, None) < 0 and b"multiple of 32" in err()
    for r in (0, 65):
        assert fwd(p, arr, arr, arr, d, 1, 4, 64, r, 1.0, None) < 0 and b"rank" in err()
    for T in (0, 65):
        assert fwd(p, arr, arr, arr, d, 1, T, 64, 16, 1.0, None) < 0 and b"T=" in err() and b"1..64" in err()
    for G in (0, 4):
        assert fwd(p, arr, arr, arr, d, G, 4, 64, 16, 1.0, None) < 0 and b"G=" in err()
    odd = (ctypes.c_void_p * 1)(0x10008)
    assert fwd(p, arr, odd, arr, d, 1, 4, 64, 16, 1.0, None) < 0 and b"16-byte aligned" in err()
    assert fwd(ctypes.c_void_p(0x10002), arr, arr, arr, d, 1, 4, 64, 16, 1.0, None) < 0 and b"16-byte aligned" in err()


def test_a_missing_library_is_an_error(monkeypatch):
    from moka_amd import _decode_lib
    monkeypatch.setattr(_decode_lib, "_lib", None)
    monkeypatch.setattr(_decode_lib, "LIB_PATH", os.path.join(ROOT, "moka_amd", "no_such_libmoka_decode.so"))
    with pytest.raises(_decode_lib.MokaError, match="no CPU / eager fallback"):
        _decode_lib.load()


def test_dispatch_predicate_single_disqualifiers(libs):
    from moka_amd import functional as F
    assert F.DECODE_FORWARD is False and isinstance(F.decode_launches, int)
    base = dict(switch_on=True, is_plain=True, dtype=BF16, dropout_ps=[0.0, 0.0], grad_recorded=False, T=4, d_in=4096,
                d_outs=[4096, 1024], r=16)
    assert F.decode_serves(**base) is True
    assert F.decode_serves(**dict(base, T=1)) and F.decode_serves(**dict(base, T=64)) and F.decode_serves(**dict(base, r=17))
    for change in (dict(switch_on=False), dict(is_plain=False), dict(dtype=F32), dict(dropout_ps=[0.0, 0.1]), dict(grad_recorded=True),
                   dict(T=65), dict(d_outs=[64] * 4)):
        assert F.decode_serves(**dict(base, **change)) is False, change


def test_only_plain_routing_is_plain():
    from moka_amd.routing import MokaRouting, StaticRouting, routing_for_samples
    cpu = torch.device("cpu")
    assert MokaRouting.is_plain is False
    plain = MokaRouting.plain(2, 1, cpu, 1)
    assert plain.is_plain is True and MokaRouting.plain(3, 5, cpu, 2).is_plain is True
    assert routing_for_samples(2, 1, [0, 1], cpu).is_plain is False
    t = torch.ones(1, 6, 1, dtype=torch.int32)
    z = torch.zeros(1, 6, 1, dtype=torch.int32)
    q = z.clone()
    q[0, 4:] = 1
    assert MokaRouting.from_avt_masks([t, z, z, q]).is_plain is False
    tb = torch.ones(1, 6, dtype=torch.bool)
    assert MokaRouting.from_vt_masks(tb, ~tb, ~tb).is_plain is False
    assert StaticRouting(plain).is_plain is False               # a captured TRAINING step's routing: never the decode kernel's
