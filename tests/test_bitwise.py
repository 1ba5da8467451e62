"""The one bit-for-bit comparator of the suite (tests/bitwise.py) bites: what it must refuse, what it must accept, and what its message names."""
import re

import numpy as np
import pytest

from bitwise import assert_same_arrays, assert_same_bits, bits, same


def nan_with(payload):
    return np.array([0x7FF8000000000000 | payload], np.uint64).view(np.float64)


def refused(got, want, **kw):
    """Both forms and `same` refuse the pair; returns the one-array form's message."""
    assert not same(got, want)
    with pytest.raises(AssertionError, match="^pair: array a"):
        assert_same_arrays(dict(a=got), dict(a=want), what="pair")
    with pytest.raises(AssertionError, match="^pair: array a"):
        assert_same_arrays(dict(a=got, b=got), dict(a=want, b=got), ("a",), "pair")
    with pytest.raises(AssertionError) as e:
        assert_same_bits(got, want, "pair", **kw)
    return str(e.value)


def test_a_different_shape_is_refused():
    msg = refused(np.zeros((2, 3)), np.zeros((3, 2)))
    assert "(2, 3)" in msg and "(3, 2)" in msg
    refused(np.zeros(4), np.zeros(5))


def test_a_different_dtype_with_equal_values_is_refused():
    got, want = np.arange(5, dtype=np.int32), np.arange(5, dtype=np.uint32)
    assert (got == want).all()
    msg = refused(got, want)
    assert "int32" in msg and "uint32" in msg
    refused(np.zeros(3, np.float32), np.zeros(3, np.uint32))                    # ... and of one size, with equal bits


def test_the_sign_of_zero_is_seen():
    got, want = np.array([1.0, -0.0, 2.0]), np.array([1.0, 0.0, 2.0])
    assert (got == want).all()
    msg = refused(got, want)
    assert "1 of 3" in msg and "first at [1]" in msg
    assert "0x8000000000000000" in msg and "-0.0" in msg


def test_nan_payloads_are_seen():
    got, want = np.concatenate([[1.0], nan_with(1)]), np.concatenate([[1.0], nan_with(2)])
    msg = refused(got, want)
    assert "1 of 2" in msg and "first at [1]" in msg
    assert "0x7ff8000000000001" in msg and "0x7ff8000000000002" in msg


@pytest.mark.parametrize("dtype", [np.uint8, np.uint32, np.float64])
def test_one_differing_element_at_the_last_index_is_found(dtype):
    want = np.arange(24).reshape(2, 3, 4).astype(dtype)
    got = want.copy()
    got[1, 2, 3] = 99
    msg = refused(got, want)
    assert "1 of 24 elements differ" in msg and "first at [1, 2, 3]" in msg
    assert re.search(r"99(\.0)?\b.* vs .*23(\.0)?\b", msg), msg
    flat = refused(got.reshape(-1), want.reshape(-1))
    assert "1 of 24" in flat and "first at [23]" in flat


def test_the_count_and_the_first_index_are_named():
    want = np.zeros(10, np.uint32)
    got = want.copy()
    got[[4, 7, 9]] = 5
    msg = refused(got, want)
    assert msg.startswith("pair: ") and "3 of 10 elements differ" in msg and "first at [4]" in msg


def test_a_missing_or_extra_key_is_refused_without_names():
    a = np.arange(3)
    with pytest.raises(AssertionError, match="set"):
        assert_same_arrays(dict(x=a), dict(x=a, y=a), what="set")               # a missing key
    with pytest.raises(AssertionError, match="set"):
        assert_same_arrays(dict(x=a, y=a), dict(x=a), what="set")               # an extra key
    assert_same_arrays(dict(x=a, y=a), dict(x=a, z=a + 1), ("x",), "set")       # with names, only the named arrays count


def test_another_dtype_than_the_one_asked_is_refused():
    a = np.arange(4, dtype=np.int64)
    assert_same_bits(a, a.copy(), "colours")
    with pytest.raises(AssertionError, match="uint32"):
        assert_same_bits(a, a.copy(), "colours", dtype=np.uint32)
    with pytest.raises(AssertionError, match="uint32"):
        assert_same_bits(a.astype(np.float32), a.astype(np.float32), "colours", dtype=np.uint32)
    assert_same_bits(a.astype(np.uint32), a.astype(np.uint32), "colours", dtype=np.uint32)


def test_equal_arrays_are_accepted():
    for a in (np.arange(7, dtype=np.uint8), np.arange(6, dtype=np.uint32).reshape(2, 3), np.linspace(-1.0, 1.0, 9), np.array([True, False]), np.zeros(0),
              np.array([np.inf, -np.inf, -0.0, 0.0]), np.float64(3.5), np.arange(4, dtype=np.int16)):
        assert same(a, a.copy())
        assert_same_bits(a, a.copy(), "equal")
        assert_same_arrays(dict(a=a), dict(a=a.copy()), what="equal")
    assert_same_bits([1.0, 2.0], np.array([1.0, 2.0]), "a list against its array")


def test_nans_with_the_same_payload_are_accepted():
    got, want = np.concatenate([nan_with(5), [2.0]]), np.concatenate([nan_with(5), [2.0]])
    assert not (got == want).all()
    assert same(got, want)
    assert_same_bits(got, want, "nan")
    assert_same_arrays(dict(a=got), dict(a=want), what="nan")


def test_a_view_is_its_contiguous_copy():
    base = np.arange(48, dtype=np.float64).reshape(6, 8)
    for view in (base[::2, 1::3], base.T, base[:, 3]):
        assert not view.flags["C_CONTIGUOUS"]
        assert same(view, np.ascontiguousarray(view))
        assert_same_bits(view, np.ascontiguousarray(view), "view")
        assert_same_arrays(dict(a=view), dict(a=np.ascontiguousarray(view)), what="view")
    assert bits(base[:, 3]).dtype == np.uint64 and bits(base[:, 3]).shape == (6,)
