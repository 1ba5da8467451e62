"""The early exit of shadow walks (render.hip, traverse / traverse_ray: `any_ok && own_slot != kNone && own_t < max_t`) against the CPU oracle.

A shadow query (raytracer.rs:164-188) uses only Some/None of Ray::intersect_with_octant_with_max_t (ray.rs:104-168).  The kernels stop a shadow
walk at the first node whose own list yields a hit with t < max_t, at any depth: every ancestor's loop breaks on the Some this node returns and hands
a t' <= t < max_t upwards, so the root returns Some.  The tempting shortcut "any hit anywhere means occluded" is NOT what the reference computes:
children are entered with max_t = +inf, the first sorted child that returns Some ends the loop, and at the root a child hit with t >= max_t and no own
hit yields None.  The scene below holds, for one point light, every class of shadow ray that tells the two rules apart:

  (a) an own hit with t < max_t at a non-root node that has children                              -> occluded, the walk stops there;
  (b) the only triangles on the ray lie beyond the light (t >= max_t), in a child subtree            -> lit;
  (c) the first sorted child returns a hit beyond the light, a LATER child holds a nearer occluder   -> lit (the ray starts in the later child, whose
      box is sorted by its exit distance; the neighbour it enters through the shared plane has the same key and the smaller index: ray.rs:146-147);
  (d) max_t = 0: the light lies exactly on the surface point, the shadow ray has no direction       -> lit.

`test_shadow_ray_classes_hold_on_the_cpu` proves from oracle.intersect and a brute-force Moller-Trumbore in numpy that each class holds at least
MIN_RAYS[class] of the rays used; it needs no GPU, so the GPU tests cannot pass vacuously.  The GPU tests compare get_ray_colours of those rays and
whole frames with the oracle in all of ALL_MODES at tolerance 0 (no specular term in the material: no pow()).  A build that stops at ANY own hit
below the root, without `own_t < max_t`, turns the rays of (b) and (c) from lit to occluded and fails them.
"""
import numpy as np
import pytest

from gpu_checks import ALL_MODES, N_THREADS, assert_walks_match, oracle_for
from lighting_scenes import (SHADOW_EXIT_CAMERA as CAMERA, SHADOW_EXIT_LIGHT_ABOVE as LIGHT_ABOVE, SHADOW_EXIT_LIGHT_ON_FLOOR as LIGHT_ON_FLOOR,
                             SHADOW_EXIT_OFFSET as OFFSET, shadow_exit_arrays as _arrays, shadow_exit_lights as _lights, shadow_exit_rays as _primary_rays)

EPS = 2.220446049250313e-16
SIZES = ((160, 120), (97, 61))
MIN_RAYS = {"a": 25, "b": 20, "c": 25, "d": 16}


def _brute_force(pos, o, d):
    """Ray::intersect_with_triangle (ray.rs:56-94) against every triangle: t per triangle, NaN where the ray misses it."""
    v1, e1, e2 = pos[:, 0], pos[:, 1] - pos[:, 0], pos[:, 2] - pos[:, 0]
    h = np.cross(d, e2); a = (e1 * h).sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = 1.0 / a; s = o - v1; u = f * (s * h).sum(1); q = np.cross(s, e1); v = f * (q @ d); t = f * (e2 * q).sum(1)
        ok = ~((a > -EPS) & (a < EPS)) & (u >= 0.0) & (u <= 1.0) & (v >= 0.0) & (u + v <= 1.0) & (t > EPS)
    return np.where(ok, t, np.nan)


def _node_depths(tree):
    depth = np.full(len(tree["first_child"]), -1); depth[0] = 0
    for n in range(len(depth)):                                                # children follow their parent in the node array
        fc = int(tree["first_child"][n])
        if fc: depth[fc:fc + 8] = depth[n] + 1
    return depth


def _own_node_of(tree, tri):
    off, idx = tree["own_off"], tree["own_idx"]
    return next(n for n in range(len(off) - 1) if tri in idx[off[n]:off[n + 1]])


def _classify(osc, A, parts, light, O, D):
    """The shadow ray of every primary ray (raytracer.rs:164-188, in the reference's arithmetic) and the classes it belongs to."""
    tree = osc.octree(); depth = _node_depths(tree)
    found = {k: [] for k in "abcd"}
    L = np.array(light)
    for i, (o, d) in enumerate(zip(O, D)):
        hit, t, u, v, tri = osc.intersect(o, d)
        assert hit and tri in parts["floor"], f"primary ray {i} does not land on the floor"
        p = o + d * t
        ro = p + np.array([0.0, 1.0, 0.0]) * OFFSET                          # the floor's shading normal is (0, 1, 0) exactly
        dirv = L - p
        max_t = float(np.sqrt(dirv[0] * dirv[0] + dirv[1] * dirv[1] + dirv[2] * dirv[2]))
        occluded = osc.intersect(ro, dirv, max_t)[0]
        free = osc.intersect(ro, dirv)                                        # the same walk with nothing cut off
        tb = _brute_force(A["pos"], ro, dirv)
        nearer, beyond = np.flatnonzero(tb < max_t), np.flatnonzero(tb >= max_t)
        if max_t == 0.0 and not occluded:
            found["d"].append(i)
        elif occluded and len(nearer) and free[0] and free[4] in nearer:
            node = _own_node_of(tree, free[4])                                # the walk returned this triangle: it stood at its node, whose own hit has t < max_t
            if depth[node] >= 1 and tree["first_child"][node] != 0:
                found["a"].append(i)
        elif not occluded and len(nearer) == 0 and len(beyond) and free[0] and depth[_own_node_of(tree, free[4])] >= 1:
            found["b"].append(i)
        elif not occluded and len(nearer) and free[0] and free[4] in beyond and depth[_own_node_of(tree, free[4])] >= 1:
            found["c"].append(i)
    return found, tree


def _checked_classes(ob):
    A, parts = _arrays()
    O, D = _primary_rays()
    out = {}
    for light in (LIGHT_ABOVE, LIGHT_ON_FLOOR):
        osc = oracle_for(ob, A, _lights(None, light), CAMERA)
        out[light], tree = _classify(osc, A, parts, light, O, D)
    assert tree["max_depth"] >= 3, f"octree only {tree['max_depth']} levels deep"
    n = {k: len(out[LIGHT_ON_FLOOR if k == "d" else LIGHT_ABOVE][k]) for k in "abcd"}
    for k in "abcd":
        assert n[k] >= MIN_RAYS[k], f"class ({k}) holds only {n[k]} rays (< {MIN_RAYS[k]}); all: {n}"
    return A, O, D, n


def test_shadow_ray_classes_hold_on_the_cpu(ob):
    _, _, _, n = _checked_classes(ob)
    print(f"\n[shadow exit] rays per class: {n} (minimum {MIN_RAYS})")


@pytest.mark.gpu
@pytest.mark.parametrize("light", [LIGHT_ABOVE, LIGHT_ON_FLOOR], ids=["light_above_floor", "light_on_floor"])
def test_shadow_exit_matches_the_oracle(rrt, ob, light):
    A, O, D, _ = _checked_classes(ob)
    sd = rrt.SceneData.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], A["materials"], A["textures"])
    lights = _lights(rrt, light)
    osc = oracle_for(ob, A, lights, CAMERA)
    colours = np.fromiter((osc.get_ray_colour(O[i], D[i]) for i in range(len(O))), np.uint32, len(O))
    if light == LIGHT_ABOVE:
        assert len(set(colours.tolist())) > 3                                   # lit and occluded receivers shade differently, on both texels
    frames = [osc.render(w, h, n_threads=N_THREADS)[0] for w, h in SIZES]
    assert_walks_match(lambda mode: rrt.RayTracer(sd, lights, rrt.Vector3d(*CAMERA), box_filter=mode), frames, SIZES, f"shadow exit, light {light}",
                       ALL_MODES, rays=(O, D, colours))
