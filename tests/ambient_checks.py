"""Helpers of the tests of ambient occlusion from kept buffers (include/rrt.h: rrt_ambient_surface): the hemisphere rays of a frame's hits, restated in numpy
from the planes of rt.surface() in the contract's operation order, the masks a shadow query gives for them, and the grey value in integer arithmetic.

Plain module, not a test module: pytest does not rewrite its asserts, so every assert here states both values in its message.  It holds no fixtures.

numpy's elementwise +, -, *, / and sqrt are IEEE operations, each rounded once and never fused; sums are written with the contract's parentheses, and cross,
length and normalised are those of surface_checks.py (engine.rs:85-103).
"""
import numpy as np

from gpu_checks import POOL, traced_rows
from surface_checks import cross, length, normalised, traced_cols

W, H = 64, 48


def table8():
    """The standard table T8: phi = 2 pi (k + 0.5) / 8, cos(theta) = (0.3, 0.6, 0.85, 0.45)[k % 4], (sin(theta) cos(phi), sin(theta) sin(phi), cos(theta))."""
    k = np.arange(8)
    phi = 2.0 * np.pi * (k + 0.5) / 8.0
    c = np.array((0.3, 0.6, 0.85, 0.45))[k % 4]
    s = np.sqrt(1.0 - c * c)
    d = np.stack([s * np.cos(phi), s * np.sin(phi), c], -1)
    d.setflags(write=False)
    return d


T8 = table8()
T8_MAX_T = 2.0


class Rays:
    """The rays of the hits of `planes` (point, normal, material as rt.surface() returns them) for the table `dirs` [n][3]:
    hit [h][w][4] bool (material < n_mats), O [n_hit][3], D [n_hit][n][3], fallback [n_hit] bool (the tangent took the length(tg) == 0 branch)."""

    def __init__(self, planes, n_mats, dirs, surface_offset=1e-4):
        dirs = np.asarray(dirs, np.float64).reshape(-1, 3)
        self.hit = planes["material"] < n_mats
        p, n = planes["point"][self.hit], planes["normal"][self.hit]
        with np.errstate(invalid="ignore", divide="ignore"):
            tg = cross(n, np.broadcast_to(np.array([0.0, 1.0, 0.0]), n.shape))                             # raytracer.rs:137-141
            self.fallback = length(tg) == 0.0
            if self.fallback.any():
                tg[self.fallback] = cross(n[self.fallback], np.broadcast_to(np.array([0.0, 0.0, 1.0]), n[self.fallback].shape))   # raytracer.rs:143-149
            tg = normalised(tg)                                                                            # raytracer.rs:151
            bt = normalised(cross(n, tg))                                                                  # raytracer.rs:152
            self.O = p + n * surface_offset
            sx, sy, sz = (dirs[:, c][None, :, None] for c in range(3))
            self.D = (tg[:, None, :] * sx + bt[:, None, :] * sy) + n[:, None, :] * sz                      # five operations per component
        self.n = len(dirs)

    def flat(self):
        """(origins, directions) of all n_hit * n rays, ray k of hit j at index j * n + k."""
        return np.repeat(self.O, self.n, 0), self.D.reshape(-1, 3)

    def plane(self, occluded):
        """occluded [n_hit * n] bool (in the order of flat()) -> the expected `occluded` plane [h][w][4] uint32: bit k of a hit, 0 elsewhere."""
        bits = (np.asarray(occluded, bool).reshape(-1, self.n).astype(np.uint64) << np.arange(self.n, dtype=np.uint64)).sum(1).astype(np.uint32)
        out = np.zeros(self.hit.shape, np.uint32)
        out[self.hit] = bits
        return out


def by_shadow_query(rt, rays, max_t):
    """The expected `occluded` plane by rt.occluded (rrt_occluded_rays) on the same rays."""
    O, D = rays.flat()
    return rays.plane(rt.occluded(O, D, max_t))


def by_oracle(osc, rays, max_t):
    """The same by Some/None of the oracle's intersector."""
    O, D = rays.flat()
    return rays.plane(np.fromiter(POOL.map(lambda i: osc.intersect(O[i], D[i], max_t)[0], range(len(O))), bool, len(O)))


def popcount(a):
    a = np.asarray(a, np.uint32)
    return sum(((a >> np.uint32(k)) & np.uint32(1)).astype(np.int64) for k in range(32))


def traced_mask(w, h, region=None):
    """[rh][rw] bool: the pixels of the region (default: the frame) that the reference traces."""
    m = np.zeros((h, w), bool)
    m[np.ix_(traced_rows(h), traced_cols(w))] = True
    x0, y0, rw, rh = region or (0, 0, w, h)
    return m[y0:y0 + rh, x0:x0 + rw]


def grey_of(occluded, material, n_mats, n, traced):
    """The grey plane by the contract's integer formula from an `occluded` plane, the material plane it was made from and the traced pixels."""
    hit = np.asarray(material) < n_mats
    open_ = np.where(hit, n - popcount(occluded), n).sum(-1)
    g = (510 * open_ + 4 * n) // (8 * n)
    return np.where(traced, g * 0x010101, 0).astype(np.uint32)


def freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


def crop(planes, region):
    x0, y0, w, h = region
    return {n: np.ascontiguousarray(a[y0:y0 + h, x0:x0 + w]) for n, a in planes.items()}
