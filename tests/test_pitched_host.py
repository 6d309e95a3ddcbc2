"""CPU self-test of tests/_pitched.py: the guard-band helper behind tests/test_gpu_abi_layout.py catches every kind of violation
it is there for.  Runs on torch CPU tensors, so the teeth of the GPU tests are shown without a GPU."""
import numpy as np
import pytest
import torch

from _pitched import VEC, Pitched, layouts, round_up

DTYPES = ["f64", "f32"]


def _data(rows, width, seed=0):
    return np.random.default_rng(seed).standard_normal((rows, width))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,width", [(1, 1), (5, 3), (7, 11), (3, 64), (2, 65)])
def test_window_round_trips_in_every_layout(dtype, rows, width):
    d = _data(rows, width).astype(np.float64 if dtype == "f64" else np.float32)
    for ld, off in [(width, 0)] + layouts(width, dtype):
        p = Pitched(dtype, data=d, ld=ld, off=off)
        assert np.array_equal(p.window(), d)
        assert p.check()
        # the data sits where the ABI will look for it: buf[start + r * ld + c]
        flat = p.buf.numpy()
        for r in range(rows):
            assert np.array_equal(flat[p.start + r * ld:p.start + r * ld + width], d[r])
        # ... and everything else is NaN: padding that reaches arithmetic poisons the result
        rest = np.ones(p.total, bool)
        for r in range(rows):
            rest[p.start + r * ld:p.start + r * ld + width] = False
        assert np.all(np.isnan(flat[rest]))
        assert rest.sum() == p.total - rows * width


@pytest.mark.parametrize("dtype", DTYPES)
def test_alignment_is_produced_as_asked(dtype):
    item = 8 if dtype == "f64" else 4
    width = 8
    got = {}
    for ld, off in layouts(width, dtype):
        p = Pitched(dtype, data=_data(4, width), ld=ld, off=off)
        assert p.ptr % 16 == (off * item) % 16  # off = 0: 16-byte aligned base; off = 1: aligned to the element only
        assert p.ptr % item == 0
        assert p.ptr == p.buf.data_ptr() + p.start * item
        got[(ld, off)] = [(p.ptr + r * ld * item) % 16 for r in range(4)]
    v = VEC[dtype]
    assert [ld for ld, off in layouts(width, dtype) if off == 0] == [width + 1, width + v, round_up(width, 64) + 64]
    assert any(x != 0 for x in got[(width + 1, 0)])  # ld % VEC != 0: rows after the first leave the 16-byte grid
    assert all(x == 0 for x in got[(width + v, 0)])  # ld % VEC == 0 and an aligned base: every row stays on it
    assert all(x == item for x in got[(width + v, 1)])  # ... and none is with the base one element off
    assert all(x == 0 for x in got[(round_up(width, 64) + 64, 0)])


def _guard_positions(p):
    first, last = p.start, p.start + (p.rows - 1) * p.ld + p.width - 1
    pos = {"one before the window": first - 1, "one after the window": last + 1, "first element": 0, "last element": p.total - 1,
           "front guard row": p.start - p.ld, "back guard row": last + p.ld}
    if p.ld > p.width and p.rows > 1:
        pos["row padding"] = p.start + p.width
        pos["last row padding"] = p.start + p.ld - 1
    return pos


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", ["input", "canary"])
def test_check_fails_for_every_kind_of_guard_write(dtype, mode):
    rows, width = 5, 6
    for ld, off in layouts(width, dtype):
        probe = Pitched(dtype, data=_data(rows, width), ld=ld, off=off)
        for name, flat in _guard_positions(probe).items():
            # a finite value, -0.0, +0.0, and NaNs that differ from the sentinel only in their payload
            other_nan = torch.tensor([probe.fresh], dtype=probe.idtype).view(probe.tdtype)[0]
            for value in (1.5, -0.0, 0.0, float("nan"), other_nan):
                p = (Pitched(dtype, data=_data(rows, width), ld=ld, off=off) if mode == "input" else
                     Pitched(dtype, rows=rows, width=width, ld=ld, off=off))
                assert p.check()
                p.buf[flat] = value
                with pytest.raises(AssertionError, match="outside the"):
                    p.check(name)
                assert list(p.violations()) == [flat], (name, value)
                r, c = p.describe(flat)
                assert not (0 <= r < rows and 0 <= c < width)


@pytest.mark.parametrize("dtype", DTYPES)
def test_writes_inside_the_window_are_allowed_and_visible(dtype):
    p = Pitched(dtype, rows=3, width=5, ld=9, off=1)
    assert p.unwritten().all() and np.all(np.isnan(p.window()))
    p.buf[p.start + 1 * p.ld + 4] = 2.0  # last column of row 1
    p.buf[p.start] = float("nan")  # a NaN result is still a write: the pre-fill is one fixed payload
    assert p.check()
    u = p.unwritten()
    assert not u[1, 4] and not u[0, 0] and u.sum() == 13
    assert p.window()[1, 4] == 2.0
    q = Pitched(dtype, rows=3, width=5, ld=9, off=1)
    assert np.array_equal(q.bits(), Pitched(dtype, rows=3, width=5).bits())  # bits() does not depend on the layout
    assert not np.array_equal(p.bits(), q.bits())


def test_integer_buffers_and_vectors():
    p = Pitched("i32", rows=1, width=7, guard=1)  # labels / counts: a vector with guards in front of and behind its ends
    assert p.ld == 7 and p.unwritten().all() and p.check()
    p.buf[p.start + 6] = 3
    assert p.check() and p.window()[0, 6] == 3
    p.buf[p.start + 7] = 0
    with pytest.raises(AssertionError):
        p.check()
    v = Pitched("f64", data=np.arange(4.0))  # a 1-D array is one row
    assert v.rows == 1 and v.width == 4 and np.array_equal(v.window()[0], np.arange(4.0))
    v.buf[v.start - 1] = 0.0
    with pytest.raises(AssertionError):
        v.check()
    with pytest.raises(AssertionError):
        Pitched("f64", data=np.zeros((2, 4)), ld=3)  # the helper itself never builds ld < width
