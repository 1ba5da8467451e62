"""Helpers of the tests of the compaction of ray batches and records (include/rrt.h: rrt_compact_rays, rrt_scatter_rays): the contract restated in numpy -- the
stable partition (np.flatnonzero of the selection), the gather, the table of dead values, the scatter -- and byte-for-byte comparisons.

Plain module, not a test module: pytest does not rewrite its asserts, so every assert here states both values in its message.  It holds no fixtures.

Doubles are compared through a uint64 view: the tail's max_t is NaN, and NaN payloads and -0.0 have to survive a gather.
"""
import numpy as np

DEAD_INDEX = 0xFFFFFFFF
SELECTS = ("hit", "mirror", "flag")                # RRT_SELECT_HIT, RRT_SELECT_MIRROR, RRT_SELECT_FLAG, in their order
# the sixteen arrays of an rrt_ray_set in its order: name -> (dtype, elements per entry, the dead value of a tail slot)
ARRAYS = {
    "origins": (np.float64, 3, (0.0, 0.0, 0.0)), "dirs": (np.float64, 3, (0.0, 0.0, 0.0)), "max_t": (np.float64, 1, (np.nan,)), "rot": (np.float64, 2, (1.0, 0.0)),
    "hit": (np.uint8, 1, (0,)), "t": (np.float64, 1, (0.0,)), "u": (np.float64, 1, (0.0,)), "v": (np.float64, 1, (0.0,)),
    "tri": (np.uint32, 1, (0xFFFFFFFF,)), "albedo": (np.uint32, 1, (0x00FFFFFF,)),
    "point": (np.float64, 3, (0.0, 0.0, 0.0)), "normal": (np.float64, 3, (0.0, 0.0, 0.0)),
    "material": (np.uint32, 1, (0xFFFFFFFF,)), "lights": (np.uint32, 1, (0,)),
    "next_origin": (np.float64, 3, (0.0, 0.0, 0.0)), "next_dir": (np.float64, 3, (0.0, 0.0, 0.0)),
}
NAMES = tuple(ARRAYS)
RECORD_NAMES = NAMES[4:]                           # the twelve arrays of rrt_ray_surface
ELEM_BYTES = {name: np.dtype(dtype).itemsize * width for name, (dtype, width, _) in ARRAYS.items()}
OFFSETS = {name: 8 * k for k, name in enumerate(NAMES)}   # of the pointer in rrt_ray_set (rec starts at 32)
NAN_BITS = 0x7FF8000000000000                      # the tail's max_t


def bits(a):
    """An array as unsigned integers of its item size, for comparisons that see NaN payloads and the sign of zero."""
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def assert_same_bytes(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.dtype}{got.shape} vs {want.dtype}{want.shape}"
    g, w = bits(got), bits(want)
    bad = g != w
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at {np.argwhere(bad)[0].tolist()}: {int(g[bad][0]):#x} vs {int(w[bad][0]):#x}"


def selection(select, n_mats=None, material=None, kr=None, flag=None):
    """sel [n] bool of rrt.h: "hit": material < n_mats; "mirror": that and kr[material] > 0.0 (kr: the table's [n_mats]); "flag": flag != 0."""
    if select == "flag":
        return np.asarray(flag) != 0
    material = np.asarray(material, np.uint32)
    hit = material < n_mats
    if select == "hit":
        return hit
    assert select == "mirror", select
    out = np.zeros(len(material), bool)
    out[hit] = np.asarray(kr, np.float64)[material[hit]] > 0.0
    return out


def dead(name, n):
    """n tail slots of array `name`."""
    dtype, width, value = ARRAYS[name]
    a = np.empty((n, width) if width > 1 else (n,), dtype)
    a[...] = np.array(value, dtype) if width > 1 else dtype(value[0])
    return a


def compacted(sel, arrays, synth_max_t=False):
    """The contract's result for the selection `sel` [n] and the source arrays {name: array}: {"index", "count", name: array}.  synth_max_t: no source bound, the
    survivors get +inf and the tail NaN."""
    sel = np.asarray(sel, bool)
    n = len(sel)
    keep = np.flatnonzero(sel)
    index = np.full(n, DEAD_INDEX, np.uint32)
    index[:len(keep)] = keep
    out = dict(index=index, count=len(keep))
    for name, a in arrays.items():
        dtype, width, _ = ARRAYS[name]
        a = np.asarray(a).reshape((n, width) if width > 1 else (n,))
        assert a.dtype == dtype, f"{name}: {a.dtype}, want {np.dtype(dtype)}"
        out[name] = np.concatenate([a[keep], dead(name, n - len(keep))])
    if synth_max_t:
        assert "max_t" not in arrays
        out["max_t"] = np.concatenate([np.full(len(keep), np.inf), dead("max_t", n - len(keep))])
    assert "max_t" not in out or n == len(keep) or int(bits(out["max_t"])[-1]) == NAN_BITS
    return out


def assert_compacted(got, want, what):
    """Every key of `want` in `got`, byte for byte; nothing else in `got`."""
    assert set(got) == set(want), f"{what}: {sorted(got)} vs {sorted(want)}"
    assert int(got["count"]) == int(want["count"]), f"{what}: count {int(got['count'])} vs {int(want['count'])}"
    for name in want:
        if name != "count":
            assert_same_bytes(np.asarray(got[name]).reshape(np.asarray(want[name]).shape), want[name], f"{what}: {name}")


def scattered(index, src, dst):
    """The contract's scatter: a copy of dst with dst[index[j]] = src[j] for every j whose index is below n.  The indices below n must be distinct."""
    index = np.asarray(index, np.uint32)
    n = len(index)
    ok = index < n
    assert len(np.unique(index[ok])) == int(ok.sum()), "the model needs distinct indices"
    out = np.array(dst, copy=True)
    out[index[ok]] = np.asarray(src)[ok]
    return out


def flag_patterns(n, seed=20240607):
    """The flag arrays of rrt.h's edge cases for a batch of n: {what: uint8 [n]}."""
    alt = (np.arange(n) & 1).astype(np.uint8)
    first, last = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    first[0] = 1
    last[-1] = 7                                    # any non-zero byte selects
    half = (np.random.default_rng(seed + n).random(n) < 0.5).astype(np.uint8)
    return {"all 0": np.zeros(n, np.uint8), "all 1": np.ones(n, np.uint8), "alternating": alt, "only the first": first, "only the last": last, "a random half": half}
