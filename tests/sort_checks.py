"""Helpers of the tests of the sort of ray batches and records by a coherence key (include/rrt.h: rrt_sort_rays): the contract restated in numpy -- the key of an
entry, one rounded f64 operation at a time; the stable ascending sort (np.argsort(kind="stable")); the gather -- and the key patterns of the edge cases.

Plain module, not a test module: pytest does not rewrite its asserts, so every assert here states both values in its message.  It holds no fixtures.

Doubles are compared through their integer bits (bitwise.assert_same_bits): NaN payloads and -0.0 have to survive a gather.
"""
import numpy as np

from bitwise import assert_same_bits
from compact_checks import ARRAYS

DEAD_KEY = 0xFFFFFFFF
KEY_MODES = ("given", "ray", "record")             # RRT_SORT_KEY_GIVEN, RRT_SORT_KEY_RAY, RRT_SORT_KEY_RECORD, in their order
CELLS = 512                                        # per axis of the root box


def root_box_of(octree):
    """(lo [3], hi [3]) of node 0 of the dict RayTracer.octree() returns."""
    box = np.asarray(octree["aabb"], np.float64).reshape(-1, 6)[0]
    return box[:3].copy(), box[3:].copy()


def ray_key(p, d, dead, root_box):
    """key [n] uint32 of rrt.h for positions p [n][3], directions d [n][3], dead [n] bool and root_box = (lo, hi): per axis s = 512.0 / (hi - lo), q = (p - lo) * s
    (each operation a rounded f64 one), cell = 511 if q >= 511.0, (uint32)q if q > 0.0, else 0 (NaN, -inf: 0); key bit 3 b + a = bit b of cell_a, key bit 27 + a =
    d.a < 0.0; a dead entry's key is 0xFFFFFFFF."""
    p, d = np.asarray(p, np.float64).reshape(-1, 3), np.asarray(d, np.float64).reshape(-1, 3)
    lo, hi = (np.asarray(v, np.float64) for v in root_box)
    key = np.zeros(len(p), np.uint32)
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(3):
            s = np.float64(512.0) / (hi[a] - lo[a])
            q = (p[:, a] - lo[a]) * s
            inner = q > 0.0
            cell = np.zeros(len(p), np.uint32)
            cell[inner] = np.minimum(q[inner], 511.0).astype(np.uint32)          # (truncation of a value in (0, 511])
            cell[q >= 511.0] = 511
            for b in range(9):
                key |= ((cell >> np.uint32(b)) & np.uint32(1)) << np.uint32(3 * b + a)
            key |= (d[:, a] < 0.0).astype(np.uint32) << np.uint32(27 + a)
    key[np.asarray(dead, bool)] = DEAD_KEY
    return key


def dead_rays(max_t, n):
    """dead [n] of the RAY mode: max_t given and not above 0 (NaN counts)."""
    if max_t is None:
        return np.zeros(n, bool)
    with np.errstate(invalid="ignore"):
        return ~(np.asarray(max_t, np.float64) > 0.0)


def sorted_batch(keys, arrays):
    """The contract's result for the keys [n] and the source arrays {name: array}: {"index", "keys", "count", name: array}."""
    keys = np.asarray(keys, np.uint32)
    n = len(keys)
    index = np.argsort(keys, kind="stable").astype(np.uint32)
    out = dict(index=index, keys=keys[index], count=int((keys != DEAD_KEY).sum()))
    for name, a in arrays.items():
        dtype, width, _ = ARRAYS[name]
        a = np.asarray(a).reshape((n, width) if width > 1 else (n,))
        assert a.dtype == dtype, f"{name}: {a.dtype}, want {np.dtype(dtype)}"
        out[name] = a[index]
    assert (out["keys"][:out["count"]] != DEAD_KEY).all() and (out["keys"][out["count"]:] == DEAD_KEY).all()
    return out


def assert_sorted(got, want, what):
    """Every key of `want` in `got`, byte for byte; nothing else in `got`."""
    assert set(got) == set(want), f"{what}: {sorted(got)} vs {sorted(want)}"
    assert int(got["count"]) == int(want["count"]), f"{what}: count {int(got['count'])} vs {int(want['count'])}"
    for name in want:
        if name != "count":
            assert_same_bits(np.asarray(got[name]).reshape(np.asarray(want[name]).shape), want[name], f"{what}: {name}")


def has_ties(keys):
    return len(np.unique(keys)) < len(keys)


def key_patterns(n, seed=20241019):
    """The key arrays of the edge cases for a batch of n: {what: uint32 [n]}."""
    rng = np.random.default_rng(seed + n)
    i = np.arange(n, dtype=np.uint64)
    r32 = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    with_dead = rng.integers(0, 2 ** 32 - 1, n, dtype=np.uint64).astype(np.uint32)
    with_dead[::11] = DEAD_KEY
    return {"all equal": np.full(n, 0x12345678, np.uint32),
            "strictly descending": (np.uint64(0xFFFFFFFE) - i * np.uint64(max(1, (2 ** 32 - 2) // max(n, 1)))).astype(np.uint32),
            "two values alternating": np.where(i & np.uint64(1), 0x00010000, 0x80000001).astype(np.uint32),
            "only the top byte differs": ((rng.integers(0, 256, n, dtype=np.uint64) << np.uint64(24)) | np.uint64(0x00ABCDEF)).astype(np.uint32),
            "only the low byte differs": (rng.integers(0, 256, n, dtype=np.uint64) | np.uint64(0x5A5A5A00)).astype(np.uint32),
            "random 32-bit": r32,
            "random in [0, 8)": rng.integers(0, 8, n, dtype=np.uint64).astype(np.uint32),
            "every 11th dead": with_dead}
