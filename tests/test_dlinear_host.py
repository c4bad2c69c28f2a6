"""CPU: the fused decode-step projection library (include/moka_dlinear.h) builds for gfx950 beside libmoka_hip.so and libmoka_decode.so
without entering either, exports what its header declares, validates its arguments on the host, reports its launch rule without a
device, and the Python dispatch rule sends it exactly the calls it is meant for."""
import ctypes
import os

import pytest

from tests.decode_util import ROOT, _declared, _ints

BF16, F32 = 0, 1
NAMES = ["moka_dlinear_fwd", "moka_dlinear_last_error", "moka_dlinear_max_tokens", "moka_dlinear_ok", "moka_dlinear_version",
         "moka_dlinear_workgroups"]


@pytest.fixture(scope="module")
def libs():
    from moka_amd import _decode_lib, _dlinear_lib, _lib, build
    path = build.build(verbose=False)          # hipcc cross-compiles without a GPU; no-op when up to date
    assert os.path.basename(path) == "libmoka_hip.so"
    return _lib.load(), _decode_lib.load(), _dlinear_lib.load()


def test_build_produces_all_three_libraries(libs):
    from moka_amd import _dlinear_lib, build
    assert os.path.exists(build.OUT) and os.path.exists(build.OUT_DECODE) and os.path.exists(build.OUT_DLINEAR)
    assert _dlinear_lib.LIB_PATH == build.OUT_DLINEAR and len({build.OUT, build.OUT_DECODE, build.OUT_DLINEAR}) == 3
    assert build.build_dlinear(verbose=False) == build.OUT_DLINEAR        # up to date: a no-op
    assert libs[2].moka_dlinear_version() == 100
    assert libs[2].moka_dlinear_max_tokens() == 16


def test_every_declared_symbol_is_exported_and_bound(libs):
    from moka_amd import _dlinear_lib
    declared = _declared("moka_dlinear.h")
    assert declared == NAMES and all(n.startswith("moka_dlinear_") for n in declared)
    for name in declared:
        assert hasattr(libs[2], name), f"{name} declared in moka_dlinear.h but not exported"
    assert sorted(_dlinear_lib.SYMBOLS) == declared
    for fn in ("load", "check", "last_error", "dlinear_ok"):
        assert callable(getattr(_dlinear_lib, fn))


def test_the_other_libraries_hold_nothing_of_it(libs):
    from moka_amd import _decode_lib, _lib, build
    for header in ("moka_hip.h", "moka_decode.h"):
        assert not [n for n in _declared(header) if "dlinear" in n]
        assert "dlinear" not in open(os.path.join(ROOT, "include", header)).read()
    assert not [n for n in list(_lib.SYMBOLS) + list(_decode_lib.SYMBOLS) if "dlinear" in n]
    for name in NAMES:
        assert not hasattr(libs[0], name), f"libmoka_hip.so exports {name}"
        assert not hasattr(libs[1], name), f"libmoka_decode.so exports {name}"
    for path in (build.OUT, build.OUT_DECODE):
        assert b"moka_dlinear" not in open(path, "rb").read(), path
    mine = {build.DLINEAR_SRC, os.path.join(ROOT, "include", "moka_dlinear.h")}
    assert mine <= set(build.dlinear_sources())
    assert not set(build.sources()) & mine and not set(build.decode_sources()) & mine
    assert not [p for p in build.sources() + build.decode_sources() if "dlinear" in os.path.basename(p)]
    assert build.UNITS == ["k_cross", "k_expand", "k_wgrad", "k_reduce", "k_misc", "moka_api"]
    assert [os.path.basename(h) for h in build.HEADERS] == ["moka_device.h", "moka_host.h", "moka_hip.h"]
    assert "dlinear" not in open(build.SRC).read()


def test_the_shared_kernel_header_belongs_to_the_two_decode_libraries_alone():
    from moka_amd import build
    step = os.path.join(ROOT, "moka_amd", "csrc", "moka_step.h")
    assert os.path.exists(step)
    assert step in build.decode_sources() and step in build.dlinear_sources()         # both libraries rebuild when it changes
    assert step not in build.sources()                                                # ... and the traffic stamp does not move
    assert "decode" not in os.path.basename(step) and "dlinear" not in os.path.basename(step)
    assert os.path.basename(step) not in open(build.SRC).read()                       # the unity file does not include it


def test_dlinear_ok_table(libs):
    ok, err = libs[2].moka_dlinear_ok, libs[2].moka_dlinear_last_error
    one = _ints([4096])
    assert [ok(T, 4096, one, 1, 16, BF16) for T in (1, 16)] == [1, 1]
    assert [ok(T, 4096, one, 1, 16, BF16) for T in (0, 17)] == [0, 0]            # valid shapes of the paths below it
    assert [ok(4, 4096, one, 1, r, BF16) for r in (1, 16, 17, 64)] == [1, 1, 1, 1]
    for r in (0, 65):
        assert ok(4, 4096, one, 1, r, BF16) < 0 and b"rank" in err()
    assert ok(4, 4096, one, 0, 16, BF16) < 0 and b"G=" in err()
    assert ok(4, 4096, _ints([64] * 4), 4, 16, BF16) < 0 and b"G=" in err()
    assert ok(4, 4096, _ints([256, 64, 64]), 3, 16, BF16) == 1
    assert ok(4, 72, one, 1, 16, BF16) < 0 and b"multiple of 32" in err()
    assert ok(4, 4096, _ints([72]), 1, 16, BF16) < 0 and b"multiple of 32" in err()
    assert ok(4, 4096, _ints([64, 72]), 2, 16, BF16) < 0
    assert ok(4, 4096, None, 1, 16, BF16) < 0 and b"null" in err()
    assert ok(4, 4096, one, 1, 16, F32) == 0
    assert ok(4, 4096, one, 1, 16, 7) < 0


def test_dlinear_fwd_validates_on_the_host(libs):
    """Every refusal comes back before a launch (this test runs without a device): fake, aligned, non-null addresses are never touched."""
    fwd, err = libs[2].moka_dlinear_fwd, libs[2].moka_dlinear_last_error
    p = ctypes.c_void_p(0x10000)
    arr = (ctypes.c_void_p * 1)(0x10000)
    null1 = (ctypes.c_void_p * 1)(None)
    odd = (ctypes.c_void_p * 1)(0x10008)
    d = _ints([64])

    def call(x=p, W=arr, bias=None, A=arr, Bw=arr, y=arr, d_out=d, G=1, T=4, d_in=64, r=16):
        return fwd(x, W, bias, A, Bw, y, d_out, G, T, d_in, r, 1.0, None)

    for kw in (dict(x=None), dict(W=None), dict(A=None), dict(Bw=None), dict(y=None), dict(d_out=None),
               dict(W=null1), dict(A=null1), dict(Bw=null1), dict(y=null1)):
        assert call(**kw) < 0 and b"null" in err(), kw
    for kw in (dict(x=ctypes.c_void_p(0x10002)), dict(W=odd), dict(A=odd), dict(Bw=odd), dict(y=odd), dict(bias=odd)):
        assert call(**kw) < 0 and b"16-byte aligned" in err(), kw
    assert call(d_in=72) < 0 and b"multiple of 32" in err()
    assert call(d_out=_ints([72])) < 0 and b"multiple of 32" in err()
    for r in (0, 65):
        assert call(r=r) < 0 and b"rank" in err()
    for T in (0, 17):
        assert call(T=T) < 0 and b"T=" in err() and b"1..16" in err()
    for G in (0, 4):
        assert call(G=G) < 0 and b"G=" in err()
    # a NULL bias array and NULL entries pass validation: with them and an otherwise valid call the next refusal is another argument's
    assert call(bias=None, T=17) < 0 and b"T=" in err()
    assert call(bias=null1, y=odd) < 0 and b"16-byte aligned" in err()
    assert call(bias=null1, y=null1) < 0 and b"null" in err()


WIDTHS = {"7b": (4096, 11008), "13b": (5120, 13824), "70b": (8192, 28672)}


def test_launch_rule_is_readable_without_a_device(libs):
    """64 columns per workgroup; doubled (to 128 at most: the registers) while that gives more than 256 workgroups, halved (to 16 at
    least) while the halved launch still has at most 256.  So: never more than 256 unless the block is at its cap of 128, where the
    count is exactly sum(ceil(d_out / 128))."""
    wg, err = libs[2].moka_dlinear_workgroups, libs[2].moka_dlinear_last_error

    def n(d_outs, d_in=4096, r=16):
        return wg(_ints(list(d_outs)), len(d_outs), d_in, r)

    def rule(d_outs):
        blocks = lambda cb: sum(-(-d // cb) for d in d_outs)    # noqa: E731
        cb = 64
        while blocks(cb) > 256 and cb < 128:
            cb *= 2
        while cb > 16 and blocks(cb // 2) <= 256:
            cb //= 2
        return blocks(cb)

    for name, (h, ff) in WIDTHS.items():
        for d_outs in ((h, h, h), (ff, ff), (h,), (h, h // 8, h // 8)):
            got = n(d_outs, d_in=h)
            promised = max(256, sum(-(-d // 128) for d in d_outs))
            print(name, d_outs, got)
            assert 1 <= got <= promised and got == rule(d_outs), (name, d_outs, got)
    assert n((4096,)) == 256 and n((4096, 4096, 4096)) == 192 and n((11008, 11008)) == 172       # 7B: o / down, q+k+v, gate+up
    assert n((28672, 28672)) == 448                                                               # 70B gate+up: more workgroups, not a wider block
    assert n((8224, 8224), d_in=64) == 130 and n((8224,), d_in=64) == 129                         # a doubled block with a partial end
    # monotone in the column count wherever the block stays the same: below the first doubling of the narrowest block, and at the cap
    for widths in (range(32, 4096 + 1, 32), range(32768 + 32, 65536, 1024)):
        counts = [n((c,)) for c in widths]
        assert counts == sorted(counts) and counts[0] >= 1
    # every column is owned: workgroups x the widest block cover the widths
    for c in (32, 96, 4128, 8224, 16416, 40000 // 32 * 32):
        assert n((c,)) * 128 >= c
    assert n((72,)) < 0 and b"multiple of 32" in err()
    assert n((64,), r=65) < 0 and b"rank" in err()
    assert wg(None, 1, 64, 16) < 0 and b"null" in err()
    assert n((64,) * 4) < 0 and b"G=" in err()


def test_a_missing_library_is_an_error(monkeypatch):
    from moka_amd import _dlinear_lib
    monkeypatch.setattr(_dlinear_lib, "_lib", None)
    monkeypatch.setattr(_dlinear_lib, "LIB_PATH", os.path.join(ROOT, "moka_amd", "no_such_libmoka_dlinear.so"))
    with pytest.raises(_dlinear_lib.MokaError, match="no CPU / eager fallback"):
        _dlinear_lib.load()


def test_dispatch_predicate_single_disqualifiers(libs):
    from moka_amd import functional as F
    assert F.DLINEAR_FORWARD is False and F.DECODE_FORWARD is False
    assert isinstance(F.dlinear_launches, int) and F.dlinear_launches == 0
    base = dict(switch_on=True, is_plain=True, dtype=BF16, dropout_ps=[0.0, 0.0], grad_recorded=False, T=4, d_in=4096,
                d_outs=[4096, 1024], r=16, weights_row_major=True, biases_ok=True)
    assert F.dlinear_serves(**base) is True
    assert F.dlinear_serves(**dict(base, T=1)) and F.dlinear_serves(**dict(base, T=16)) and F.dlinear_serves(**dict(base, r=17))
    for change in (dict(switch_on=False), dict(is_plain=False), dict(dtype=F32), dict(dropout_ps=[0.0, 0.1]), dict(grad_recorded=True),
                   dict(T=17), dict(T=0), dict(d_outs=[64] * 4), dict(weights_row_major=False), dict(biases_ok=False), dict(r=65),
                   dict(d_in=72)):
        assert F.dlinear_serves(**dict(base, **change)) is False, change
