"""Helpers of the tests of the compaction of ray batches and records (include/rrt.h: rrt_compact_rays, rrt_scatter_rays): the contract restated in numpy -- the
stable partition (np.flatnonzero of the selection), the gather, the table of dead values, the scatter -- compared bit for bit (bitwise.py), and the device
buffers the compaction, sort and counted tests pass to the library: to_device, Guarded outputs between guard elements, ceil_div, mixed_waves.

Plain module, not a test module: pytest does not rewrite its asserts, so every assert here states both values in its message.  It holds no fixtures.

Doubles are compared through their integer bits: the tail's max_t is NaN, and NaN payloads and -0.0 have to survive a gather.
"""
import numpy as np

from bitwise import assert_same_bits, bits

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
G = 64                                             # guard elements on both sides of a device output
# the batch sizes of the scratch-size tests of compaction and sorting: the edge sizes of tests/test_gpu_compact.py, and 2^16, 2^20
SCRATCH_SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2047, 2049, 4097, 70001, 2 ** 16, 2 ** 20, 2 ** 20 + 4097)


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
            assert_same_bits(np.asarray(got[name]).reshape(np.asarray(want[name]).shape), want[name], f"{what}: {name}")


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


# ------------------------------------------------------------------ device buffers (torch is the caller's: this module imports none)
def ceil_div(a, b):
    return -(-a // b)


def mixed_waves(sel):
    """The number of whole 64-entry waves of a batch that hold both selected and unselected entries."""
    w = np.asarray(sel, bool)[:len(sel) // 64 * 64].reshape(-1, 64)
    return int((w.any(1) & ~w.all(1)).sum())


def torch_dtype(torch, dtype):
    return {np.dtype(np.float64): torch.float64, np.dtype(np.uint32): torch.int32, np.dtype(np.uint8): torch.uint8}[np.dtype(dtype)]


def to_device(torch, a):
    """A host array as a flat device tensor of the same bits (uint32 travels as int32)"""
    a = np.ascontiguousarray(a)
    return torch.tensor(a.view(np.int32) if a.dtype == np.uint32 else a, device="cuda").reshape(-1)


class Guarded:
    """A device output of `count` elements of `dtype` between G guard elements of 0xA5 bytes on both sides."""

    def __init__(self, torch, dtype, count):
        self.dtype, self.size = np.dtype(dtype), np.dtype(dtype).itemsize
        self.raw = torch.full(((2 * G + count) * self.size,), 0xA5, dtype=torch.uint8, device="cuda")
        self.t = self.raw[G * self.size:(G + count) * self.size].view(torch_dtype(torch, dtype))

    def read(self, what):
        a = self.raw.cpu().numpy()
        g = G * self.size
        assert (a[:g] == 0xA5).all() and (a[len(a) - g:] == 0xA5).all(), f"{what}: an element outside the output was written"
        return a[g:len(a) - g].view(self.dtype).copy()

    def untouched(self):
        return bool((self.raw == 0xA5).all().item())
