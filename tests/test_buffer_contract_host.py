"""tests/arena.py on CPU tensors: every deliberate mistake a kernel could make is flagged, a correct call passes."""
import pytest
import torch

from tests.arena import Arena, Buf, ContractError, guard_bytes

bf = torch.bfloat16


def _arena(shift=0):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(37, 96, generator=g).to(bf)
    acc = torch.randn(16, 96, generator=g)
    zero = torch.zeros(40, 32, dtype=torch.bool)
    zero[37:] = True                                     # token padding rows
    zero[:, 24:] = True                                  # rank padding columns
    spec = {
        "x": Buf((37, 96), bf, "input", data=x),
        "out": Buf((40, 32), torch.float32, "write", zero=zero),
        "acc": Buf((16, 96), torch.float32, "inout", data=acc),
        "keep": Buf((37, 96), torch.uint8, "write"),
        "ws": Buf((1000,), torch.uint8, "workspace"),
    }
    return Arena("cpu", spec, shift=shift), x, acc


def _correct_call(a, x, acc):
    out = a.view("out")
    out.zero_()
    out[:37, :24] = x.float()[:, :24] * 2
    a.view("acc").add_(x.float()[:16] * 0.5)
    a.view("keep").copy_((x > 0).to(torch.uint8))
    a.view("ws").fill_(7)


@pytest.mark.parametrize("shift", [0, 144])
def test_a_correct_call_passes_and_accumulators_come_back_as_deltas(shift):
    a, x, acc = _arena(shift)
    for name in a.spec:
        assert (a.ptr(name) - a.mem.data_ptr()) % 256 == shift
    _correct_call(a, x, acc)
    a.check()
    assert torch.allclose(a.delta("acc"), x.double()[:16] * 0.5, atol=1e-6)
    assert a.check_delta("acc", x.double()[:16] * 0.5, 1e-6) < 1e-6
    assert torch.equal(a.prior("acc"), acc)


def test_guard_size_covers_a_token_block_and_a_chunk():
    wide = Buf((8, 11008), bf, "input", data=torch.zeros(8, 11008))
    g = guard_bytes([wide])
    assert g >= 1 << 20 and g >= 128 * 11008 * 2 + 512 * 2 and g % 256 == 0


def test_input_guards_hold_nan_and_output_guards_a_seeded_pattern():
    a, _, _ = _arena()
    g0, start, _, _ = a.place["x"]
    assert torch.isnan(a.mem[start - 64:start].view(bf)).all()
    _, start, _, _ = a.place["out"]
    b, _, _ = _arena()
    assert torch.equal(a.mem[start - 64:start], b.mem[start - 64:start])      # fixed, seeded
    assert int(a.mem[start - 4096:start].unique().numel()) > 200              # not a constant


def _raises(a, pattern):
    with pytest.raises(ContractError, match=pattern):
        a.check()


def _raw(a, name):
    """The whole allocation as elements of `name`'s type, and the element index of `name`'s first element in it."""
    b = a.spec[name]
    start = a.place[name][1]
    return a.mem.view(b.dtype), start // b.esize


def test_flags_one_element_written_past_the_end():
    a, x, acc = _arena()
    _correct_call(a, x, acc)
    flat, s = _raw(a, "out")
    flat[s + 40 * 32] = 1.0
    _raises(a, r"out: written past the end \(elements 0\.\.0")
    assert a.guard_damage() == [("out", "after", 0, 0)]


def test_flags_one_element_written_before_the_start():
    a, x, acc = _arena()
    _correct_call(a, x, acc)
    flat, s = _raw(a, "acc")
    flat[s - 1] += 1.0
    _raises(a, r"acc: written before the start \(elements 0\.\.0")


def test_flags_a_nan_left_in_a_write_buffer():
    a, x, acc = _arena()
    _correct_call(a, x, acc)
    a.view("out")[5, 3] = float("nan")
    _raises(a, r"out: 1 element\(s\) never written \(first at \[5, 3\]\)")


def test_flags_an_unwritten_byte_output():
    a, x, acc = _arena()
    _correct_call(a, x, acc)
    a.view("keep")[36, 95] = 0xA5
    _raises(a, r"keep: 1 element\(s\) never written")


def test_exempt_elements_may_stay_unwritten():
    a, x, acc = _arena()
    a.spec["out"].exempt = torch.zeros(40, 32, dtype=torch.bool)
    a.spec["out"].exempt[7] = True
    _correct_call(a, x, acc)
    a.view("out")[7, :24] = float("nan")
    a.check()


def test_flags_a_non_zero_padding_element():
    a, x, acc = _arena()
    _correct_call(a, x, acc)
    a.view("out")[38, 0] = 1e-30                         # a token padding row
    _raises(a, r"out: 1 padding element\(s\) not zero \(first at \[38, 0\]\)")
    a2, x, acc = _arena()
    _correct_call(a2, x, acc)
    a2.view("out")[0, 31] = -2.0                         # a rank padding column
    _raises(a2, r"padding element")


def test_an_overwritten_accumulator_shows_in_the_delta():
    a, x, acc = _arena()
    _correct_call(a, x, acc)
    a.view("acc").copy_(x.float()[:16] * 0.5)            # `=` instead of `+=`
    a.check()                                            # nothing structural is wrong ...
    with pytest.raises(ContractError, match=r"acc: after - before is .* away from the expected increment"):
        a.check_delta("acc", x.double()[:16] * 0.5, 1e-5)   # ... but the increment is off by the prior


def test_flags_a_modified_input():
    a, x, acc = _arena()
    _correct_call(a, x, acc)
    a.view("x")[10, 10] = -a.view("x")[10, 10] + 1
    _raises(a, r"x: input modified \(\d+ bytes changed\)")


def test_a_workspace_may_be_written_but_not_past_its_end():
    a, x, acc = _arena()
    _correct_call(a, x, acc)
    a.check()
    flat, s = _raw(a, "ws")
    flat[s + 1000 + 17] ^= 0xFF
    _raises(a, r"ws: written past the end \(elements 17\.\.17")


def test_several_problems_are_reported_together():
    a, x, acc = _arena()
    _correct_call(a, x, acc)
    a.view("x")[0, 0] = 5.0
    a.view("out")[0, 0] = float("nan")
    with pytest.raises(ContractError) as e:
        a.check()
    assert "x: input modified" in str(e.value) and "out: 1 element(s) never written" in str(e.value)
