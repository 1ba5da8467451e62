"""Helpers of the tests of ambient occlusion for ray records (include/rrt.h: rrt_ambient_rays): the hemisphere fan of a record set, restated in numpy from the
arrays of rt.surface_rays() in the contract's operation order -- with and without a rotation per record -- the masks a shadow query gives for it, and `open`; and the level-1 record set of the teapot frame that the
ambient, compaction and sort tests share (level1, and the fixture kept_records).

Plain module, not a test module: pytest does not rewrite its asserts, so every assert here states both values in its message.  Its one fixture, kept_records, has module scope and requests
scenes.teapot_arrays: a test module imports both by name.

numpy's elementwise +, -, *, / and sqrt are IEEE operations, each rounded once and never fused; sums are written with the contract's parentheses, and cross,
length and normalised are those of surface_checks.py (engine.rs:85-103).  The class has the shape of ambient_checks.Rays: hit, O, D, fallback, flat(), plane().
"""
import numpy as np
import pytest

from ambient_checks import H, T8, T8_MAX_T, W, freeze, popcount
from gpu_checks import POOL
from scenes import CREATION, rays_of
from surface_checks import cross, length, normalised

INPUTS = ("point", "normal", "material")          # what rrt_ambient_rays reads of an rrt_ray_surface
OUTPUTS = ("occluded", "open")                    # rrt_ray_ambient, in its order
GOLDEN = 0.6180339887498949                       # frac of the golden ratio


def standard_rot(n):
    """ROT(i) = (cos a, sin a), a = 2 pi frac(i * 0.6180339887498949), for i in [0, n): [n][2], read-only."""
    a = 2.0 * np.pi * np.modf(np.arange(n, dtype=np.float64) * GOLDEN)[0]
    r = np.ascontiguousarray(np.stack([np.cos(a), np.sin(a)], -1))
    r.setflags(write=False)
    return r


class Fan:
    """The rays of the hits of the records `rec` (point [n][3], normal [n][3], material [n] as rt.surface_rays() returns them) for the table `dirs` [k][3] and
    the rotations `rot` ([n][2] of (c, s), or None):
    hit [n] bool (material < n_mats), O [n_hit][3], D [n_hit][k][3], fallback [n_hit] bool (the tangent took the length(tg) == 0 branch)."""

    def __init__(self, rec, n_mats, dirs, rot=None, surface_offset=1e-4):
        dirs = np.asarray(dirs, np.float64).reshape(-1, 3)
        material = np.asarray(rec["material"]).reshape(-1)
        self.hit = material < n_mats
        p, n = np.asarray(rec["point"], np.float64).reshape(-1, 3)[self.hit], np.asarray(rec["normal"], np.float64).reshape(-1, 3)[self.hit]
        with np.errstate(invalid="ignore", divide="ignore"):
            tg = cross(n, np.broadcast_to(np.array([0.0, 1.0, 0.0]), n.shape))                             # raytracer.rs:137-141
            self.fallback = length(tg) == 0.0
            if self.fallback.any():
                tg[self.fallback] = cross(n[self.fallback], np.broadcast_to(np.array([0.0, 0.0, 1.0]), n[self.fallback].shape))   # raytracer.rs:143-149
            tg = normalised(tg)                                                                            # raytracer.rs:151
            bt = normalised(cross(n, tg))                                                                  # raytracer.rs:152
            self.O = p + n * surface_offset
            sx, sy, sz = (dirs[:, c][None, :] for c in range(3))                                           # [1][k]
            if rot is not None:
                r = np.asarray(rot, np.float64).reshape(-1, 2)[self.hit]
                c, s = r[:, 0][:, None], r[:, 1][:, None]                                                  # [n_hit][1]
                sx, sy = sx * c - sy * s, sx * s + sy * c                                                  # six operations, each rounded on its own
            sx, sy, sz = (np.broadcast_to(a, (len(p), len(dirs)))[:, :, None] for a in (sx, sy, sz))
            self.D = (tg[:, None, :] * sx + bt[:, None, :] * sy) + n[:, None, :] * sz                      # five operations per component
        self.n = len(dirs)

    def flat(self):
        """(origins, directions) of all n_hit * k rays, ray k of hit j at index j * n + k."""
        return np.repeat(self.O, self.n, 0), np.ascontiguousarray(self.D).reshape(-1, 3)

    def plane(self, occluded):
        """occluded [n_hit * k] bool (in the order of flat()) -> the expected `occluded` array [n] uint32: bit k of a hit, 0 elsewhere."""
        bits = (np.asarray(occluded, bool).reshape(-1, self.n).astype(np.uint64) << np.arange(self.n, dtype=np.uint64)).sum(1).astype(np.uint32)
        out = np.zeros(self.hit.shape, np.uint32)
        out[self.hit] = bits
        return out


def by_shadow_query(rt, fan, max_t):
    """The expected `occluded` array by rt.occluded (rrt_occluded_rays) on the same rays."""
    O, D = fan.flat()
    return fan.plane(rt.occluded(O, D, max_t))


def by_oracle(osc, fan, max_t):
    """The same by Some/None of the oracle's intersector."""
    O, D = fan.flat()
    return fan.plane(np.fromiter(POOL.map(lambda i: osc.intersect(O[i], D[i], max_t)[0], range(len(O))), bool, len(O)))


def open_of(occluded, hit, n):
    """`open` by the contract from a mask: n - popcount for a hit, n for a miss or a dead record."""
    return np.where(hit, n - popcount(occluded), n).astype(np.uint32)


def mask_figures(mask, fan):
    """(occluded fraction of all rays, per-sample occluded fraction [k]) over the hits, from an `occluded` array."""
    m = np.asarray(mask)[fan.hit]
    per = np.array([float(((m >> np.uint32(k)) & np.uint32(1)).mean()) for k in range(fan.n)])
    return float(popcount(m).sum()) / (m.size * fan.n), per


def rows(rec, sel):
    """The records `sel` (a slice, indices or a bool array) of the three input arrays, contiguous."""
    return {n: np.ascontiguousarray(np.asarray(rec[n])[sel]) for n in INPUTS}


# ------------------------------------------------------------------ the record sets the tests share
def level1(rt, cam, w, h):
    """(level-0 arrays of the w x h frame's primary rays, the level-1 records of ALL its level-0 hits: INPUTS of rrt_surface_rays on their next_origin / next_dir)"""
    O, D = rays_of(cam, w, h)
    l0 = rt.surface_rays(O, D, planes=("hit", "next_origin", "next_dir"))
    h0 = l0["hit"].astype(bool)
    rec = rt.surface_rays(np.ascontiguousarray(l0["next_origin"][h0]), np.ascontiguousarray(l0["next_dir"][h0]), planes=INPUTS)
    freeze(*rec.values())
    return l0, rec


@pytest.fixture(scope="module")
def kept_records(rrt, teapot, teapot_arrays):
    """The level-1 records of the teapot's 64 x 48 frame at the creation pose and what the tests share of them (read-only): the raytracer in the default mode, the
    level-0 arrays, the level-1 records, ROT, the fans without and with it, and the masks of T8 at max_t 2.0 by rt.occluded for both."""
    rt = rrt.RayTracer(teapot, rrt.default_lights())
    l0, rec = level1(rt, CREATION, W, H)
    n_mats = len(teapot_arrays["materials"])
    rot = standard_rot(len(rec["material"]))
    fans = {False: Fan(rec, n_mats, T8), True: Fan(rec, n_mats, T8, rot)}
    want = {r: by_shadow_query(rt, fans[r], T8_MAX_T) for r in (False, True)}
    freeze(*want.values(), *l0.values())
    return dict(rt=rt, l0=l0, rec=rec, rot=rot, fans=fans, want=want, n_mats=n_mats)
