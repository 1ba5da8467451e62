"""Helpers of the tests of the deferred stages over a device-resident tile list (include/rrt.h: rrt_render_visibility_tile_list_device,
rrt_render_surface_tile_list_device, rrt_shade_surface_tile_list_device, rrt_ambient_surface_tile_list_device): whole-frame planes in guarded device buffers
prefilled with 0xA5 bytes, the plane a stage must leave in such a buffer for a list, the lists the tests run, and the sample tables.

Plain module, not a test module: pytest does not rewrite its asserts, so every assert here states both values in its message.  It holds no fixtures.
"""
import numpy as np

from ambient_checks import T8
from bitwise import assert_same_bits
from region_render_checks import listed_pixels, tiles_of

FILL = 0xA5                                               # every byte of an output before a call
TAIL = 256                                                # guard bytes behind every output
DEAD = 0xFFFFFFFF

# plane -> (dtype, elements per pixel, trailing shape): the whole-frame planes of rrt_visibility, rrt_surface and rrt_ambient, and the framebuffer
PLANES = {"hit": (np.uint8, (4,)), "t": (np.float64, (4,)), "u": (np.float64, (4,)), "v": (np.float64, (4,)), "tri": (np.uint32, (4,)), "albedo": (np.uint32, (4,)),
          "point": (np.float64, (4, 3)), "normal": (np.float64, (4, 3)), "material": (np.uint32, (4,)), "lights": (np.uint32, (4,)),
          "occluded": (np.uint32, (4,)), "grey": (np.uint32, ()), "fb": (np.uint32, ())}
VIS = ("hit", "t", "u", "v", "tri", "albedo")
SURF = ("point", "normal", "material", "lights")
TEN = VIS + SURF
SHADE_IN = ("point", "normal", "material", "albedo", "lights")
AMB_IN = ("point", "normal", "material")


def table32():
    """32 directions whose first eight are ambient_checks.T8: the other 24 by T8's rule on a finer ring, phi = 2 pi (k + 0.5) / 24 with
    cos(theta) = (0.2, 0.5, 0.7, 0.9, 0.35, 0.8)[k % 6]."""
    k = np.arange(24)
    phi = 2.0 * np.pi * (k + 0.5) / 24.0
    c = np.array((0.2, 0.5, 0.7, 0.9, 0.35, 0.8))[k % 6]
    s = np.sqrt(1.0 - c * c)
    d = np.concatenate([T8, np.stack([s * np.cos(phi), s * np.sin(phi), c], -1)])
    d.setflags(write=False)
    return d


T32 = table32()
T1 = T8[2:3]                                              # one direction: the steepest of T8


def plane_shape(name, w, h):
    return (h, w) + PLANES[name][1]


def prefill(name, w, h):
    """A whole-frame plane whose every byte is FILL."""
    a = np.empty(plane_shape(name, w, h), PLANES[name][0])
    a.view(np.uint8).fill(FILL)
    return a


def torch_kind(torch, name):
    """The torch dtype of a plane: unsigned types as the signed type of their width."""
    return {np.dtype(np.uint8): torch.uint8, np.dtype(np.uint32): torch.int32, np.dtype(np.float64): torch.float64}[np.dtype(PLANES[name][0])]


def device_plane(torch, name, w, h):
    """A whole-frame plane of zeros in device memory, shaped as the plane."""
    return torch.zeros(plane_shape(name, w, h), dtype=torch_kind(torch, name), device="cuda")


class GuardedPlane:
    """A whole-frame plane in device memory in front of TAIL guard bytes, every byte FILL.  `t` is the tensor a call takes, shaped as the plane."""

    def __init__(self, torch, name, w, h):
        self.name, self.shape, self.dtype = name, plane_shape(name, w, h), np.dtype(PLANES[name][0])
        self.bytes = prefill(name, w, h).nbytes
        self.all = torch.from_numpy(np.full(self.bytes + TAIL, FILL, np.uint8)).cuda()
        self.t = self.all[:self.bytes].view(torch_kind(torch, name)).view(self.shape)

    def host(self, what):
        """The plane, after the check that the tail still holds the guard."""
        got = self.all.cpu().numpy()
        assert (got[self.bytes:] == FILL).all(), f"{what}: plane {self.name} was written behind its end"
        return got[:self.bytes].copy().view(self.dtype).reshape(self.shape)


def guarded(torch, names, w, h):
    """{plane: GuardedPlane}"""
    return {n: GuardedPlane(torch, n, w, h) for n in names}


def tensors(planes):
    return {n: p.t for n, p in planes.items()}


def listed_only(name, full, mask):
    """The plane a stage leaves in a prefilled buffer: `full` at the pixels of mask ([h][w] bool), FILL bytes everywhere else."""
    h, w = mask.shape
    out = prefill(name, w, h)
    out[mask] = np.asarray(full)[mask]
    return out


def assert_listed_only(planes, full, w, h, tiles, what):
    """Every GuardedPlane of `planes` equals full[plane] inside the tiles the list names and still holds FILL bytes everywhere else, tail included."""
    mask = listed_pixels(w, h, tiles)
    for n, p in planes.items():
        assert_same_bits(p.host(what), listed_only(n, full[n], mask), f"{what}: plane {n}, {int(mask.sum())} listed pixels", PLANES[n][0])
    return int(mask.sum())


def inputs_for(torch, names, full, w, h, tiles):
    """{plane: device tensor}: the kept planes a shade or ambient call reads, with FILL bytes at every pixel outside the listed tiles -- what the call may not read
    (a material of 0xA5A5A5A5 is a miss, so a lane that read it would write a miss's value)."""
    mask = listed_pixels(w, h, tiles)
    return {n: torch.from_numpy(as_signed(listed_only(n, full[n], mask))).cuda() for n in names if n in full}


def as_signed(a):
    """A writable copy of a host array as torch takes it: uint32 as int32 of the same bits."""
    a = np.array(a, copy=True, order="C")
    return a.view(np.int32) if a.dtype == np.uint32 else a


def device_list(torch, tiles):
    """The list as a device tensor of its length (the empty list: a slice of length 0 of a one-entry tensor)."""
    tiles = np.asarray(tiles, np.uint32)
    host = np.full(max(len(tiles), 1), DEAD, np.uint32)
    host[:len(tiles)] = tiles
    return torch.from_numpy(host.view(np.int32)).cuda()[:len(tiles)]


def lists_of(w, h, seed=5):
    """{name: uint32 list} of the lists every stage runs on a w x h frame."""
    tx, ty = tiles_of(w, h)
    n = tx * ty
    every = np.arange(n, dtype=np.uint32)
    rng = np.random.default_rng(seed)
    quarter = rng.permutation(n)[:max(n // 4, 1)].astype(np.uint32)
    grid = every.reshape(ty, tx)
    rim = np.concatenate([grid[0, [0, tx - 1]], grid[ty - 1, [0, tx - 1]], grid[0, 1:tx - 1], grid[ty - 1, 1:tx - 1], grid[1:ty - 1, 0], grid[1:ty - 1, tx - 1]]).astype(np.uint32)
    twice = np.concatenate([quarter[:max(len(quarter) // 2, 1)], quarter[:max(len(quarter) // 2, 1)][::-1], quarter[:1]]).astype(np.uint32)
    bad = np.array([DEAD, n, n + 1], np.uint32)
    mixed = np.stack([quarter, bad[np.arange(len(quarter)) % 3]], -1).reshape(-1).astype(np.uint32)
    return {"every tile, ascending": every, "every tile, descending": every[::-1].copy(), "a seeded quarter": quarter, "the corners and the edges": rim,
            "duplicates": twice, "invalid entries interleaved": mixed, "the empty list": np.zeros(0, np.uint32)}
