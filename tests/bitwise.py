"""The suite's one bit-for-bit comparison (numpy only): bits, same, assert_same_bits for one array, assert_same_arrays for a dict of arrays.

Equal means equal shape, equal dtype and equal integer bits: two NaNs are equal only with the same payload, and -0.0 is not 0.0.  Plain module, not a
test module: pytest does not rewrite its asserts, so every assert here states both values in its message.  tests/test_bitwise.py proves that it bites.
"""
import numpy as np

UNSIGNED = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def bits(a):
    """An array as unsigned integers of its element size: equality of these is equality bit for bit (NaN payloads and the sign of zero included)."""
    a = np.ascontiguousarray(a)
    return a.view(UNSIGNED[a.dtype.itemsize])


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool((bits(a) == bits(b)).all())


def assert_same_bits(got, want, what, dtype=None):
    """got is want bit for bit, with shape and dtype (and with dtype given, both are of that dtype)."""
    got, want = np.asarray(got), np.asarray(want)
    assert dtype is None or got.dtype == want.dtype == np.dtype(dtype), f"{what}: {got.dtype}{got.shape} vs {want.dtype}{want.shape}, both must be {np.dtype(dtype)}"
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.dtype}{got.shape} vs {want.dtype}{want.shape}"
    g, w = bits(got), bits(want)
    bad = g != w
    if bad.any():
        first = tuple(np.argwhere(bad)[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at {list(first)}: "
                             f"{got[first]!r} ({int(g[first]):#x}) vs {want[first]!r} ({int(w[first]):#x})")


def assert_same_arrays(got, want, names=None, what="arrays"):
    """The arrays `names` of the dicts got and want are the same bit for bit; without names, the two hold the same keys and every array is."""
    if names is None:
        assert set(got) == set(want), f"{what}: arrays {sorted(got)} vs {sorted(want)}"
        names = list(want)
    for n in names:
        assert_same_bits(got[n], want[n], f"{what}: array {n}")
