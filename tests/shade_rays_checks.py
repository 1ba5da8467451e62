"""Helpers of the tests of shading arbitrary rays from kept records (include/rrt.h: rrt_shade_rays): the names and sentinels of its arrays, the oracle's colours of a
ray batch, a reflection chain kept level by level, and the reference's unwind (raytracer.rs:89-101) from the call's `local` and `kr`.

Plain module, not a test module: pytest does not rewrite its asserts, so every assert here states both values in its message.  It holds no fixtures.
"""
import numpy as np

from conftest import channels
from gpu_checks import POOL
from ray_surface_checks import WHITE, clamp_u8, kr_of, pack

INPUTS = ("point", "normal", "material", "albedo", "lights")     # what rrt_shade_rays reads of an rrt_ray_surface; lights is optional
OUTPUTS = ("colour", "local", "kr")                               # rrt_ray_shade, in its order
OUT_DTYPES = dict(colour=np.uint32, local=np.float64, kr=np.float64)
OUT_SENTINEL = dict(colour=-1515870811, local=-12345.5, kr=-12345.5)


def oracle_colours(osc, O, D):
    """get_ray_colour of the oracle for every ray (O[i], D[i]); O may be one point"""
    D = np.ascontiguousarray(D, np.float64).reshape(-1, 3)
    O = np.ascontiguousarray(np.broadcast_to(np.asarray(O, np.float64).reshape(-1, 3), D.shape))
    return np.fromiter(POOL.map(lambda i: osc.get_ray_colour(O[i], D[i]), range(len(D))), np.uint32, len(D))


def without_mask(planes):
    return {n: a for n, a in planes.items() if n != "lights"}


def mixed(local, kr, below):
    """raytracer.rs:89-101: local * (1 - kr) + reflected * kr per channel, clamped and truncated; numpy's multiply and add are the kernel's"""
    return pack(clamp_u8(local * (1.0 - kr)[:, None] + channels(below).astype(np.float64) * kr[:, None]))


def reflecting(A, planes, depth, max_depth):
    """The rays of a level at `depth` at which the reference reflects (raytracer.rs:76)"""
    return planes["hit"].astype(bool) & (kr_of(A, planes["material"]) > 0.0) & (depth < max_depth)


def chain_levels(rt, A, O, D, max_depth=5):
    """The reflection chain of the rays (O, D) from RayTracer.surface_rays, compacted: [(origins, directions, the twelve arrays, reflecting rays)] for the levels
    0 .. max_depth at most; the next level's rays are next_origin / next_dir of the reflecting ones."""
    levels = []
    o, d = np.ascontiguousarray(O, np.float64).reshape(-1, 3), np.ascontiguousarray(D, np.float64).reshape(-1, 3)
    for depth in range(max_depth + 1):
        planes = rt.surface_rays(o, d)
        go = reflecting(A, planes, depth, max_depth)
        levels.append((o, d, planes, go))
        if not go.any():
            break
        o, d = planes["next_origin"][go], planes["next_dir"][go]
    return levels


def unwind(levels, shade_level):
    """The colours of level 0 from shade_level(k, directions, arrays) -> (local, kr) of every level, by the rule of rrt.h alone: WHITE for a ray without a
    material, the clamped `local` where kr == 0.0, the mix with the colours of the level below where kr > 0.0."""
    below = None
    for k in reversed(range(len(levels))):
        o, d, planes, go = levels[k]
        local, kr = shade_level(k, d, planes)
        assert ((kr > 0.0) == go).all(), f"level {k}: kr > 0 on {int((kr > 0.0).sum())} rays, the reference reflects at {int(go.sum())}"
        c = np.where(planes["hit"].astype(bool), pack(clamp_u8(local)), np.uint32(WHITE)).astype(np.uint32)
        if go.any():
            c[go] = mixed(local[go], kr[go], below)
        below = c
    return below
