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

from gpu_checks import ALL_MODES, N_THREADS, ROOT_BOX, assert_walks_match, checker, oracle_for, quad

EPS = 2.220446049250313e-16
OFFSET = 1e-4                                            # SURFACE_OFFSET, raytracer.rs:17
LIGHT_ABOVE = (-2.0, -2.75, 6.0)                         # classes (a), (b), (c): a quarter above the floor
LIGHT_ON_FLOOR = (3.0, -3.0, 7.0)                        # class (d): a point of the floor that rays hit exactly
CAMERA = (0.0, 2.0, -10.0)
SIZES = ((160, 120), (97, 61))
MIN_RAYS = {"a": 25, "b": 20, "c": 25, "d": 16}


def _arrays():
    """Floor y = -3 (root list: it straddles the root's planes) and, in the root's children 1 (x < 0, y < 0, z > 0) and 2 (x > 0, y < 0, z > 0):
    FAR, a wall at x = -19 that straddles child 1's z plane (own list of a depth-1 node with children); ROOF, a ceiling at y = -2 over the light
    (own list of a depth-2 node); NEAR, a low wall at x = 1 in child 2; and two pairs of small triangles that open deeper levels."""
    groups = {"floor": quad((-16, -3, -16), (16, -3, -16), (16, -3, 16), (-16, -3, 16)),
              "far": quad((-19, -3.5, 1), (-19, -3.5, 11), (-19, -0.5, 11), (-19, -0.5, 1)),
              "roof": quad((-4.9, -2, 3), (-0.1, -2, 3), (-0.1, -2, 9), (-4.9, -2, 9)),
              "near": quad((1, -3.4, 4.5), (1, -3.4, 7.5), (1, -2.5, 7.5), (1, -2.5, 4.5)),
              "deep": [[(-7, -8, 2), (-6.8, -8, 2), (-7, -7.8, 2)], [(-7.3, -8, 2.2), (-7.1, -8, 2.2), (-7.3, -7.8, 2.2)],
                       [(7, -8, 2), (7.2, -8, 2), (7, -7.8, 2)], [(7.3, -8, 2.2), (7.5, -8, 2.2), (7.3, -7.8, 2.2)]]}
    names = [n for n, g in groups.items() for _ in g]
    pos = np.asarray([t for g in groups.values() for t in g], np.float64)
    nrm = np.tile([0.0, 1.0, 0.0], (len(pos), 3, 1))                        # the rays below only ever shade the floor
    uv = np.zeros_like(pos); uv[..., 0] = pos[..., 0] * 0.13 + pos[..., 2] * 0.07; uv[..., 1] = pos[..., 1] * 0.11 + pos[..., 2] * 0.05
    mats = [dict(ka=(1, 1, 1), kd=(1, 1, 1), ks=(0, 0, 0), ns=-1.0, kr=0.0, tex=0, bump=-1)]
    A = dict(pos=pos, uv=uv, nrm=nrm, mat=np.zeros(len(pos), np.uint32), materials=mats, textures=[checker((230, 200, 170), (120, 140, 160))], root=ROOT_BOX)
    return A, {n: np.flatnonzero(np.array(names) == n) for n in groups}


def _primary_rays():
    """Straight down onto the floor from y = -2.6 (under the roof).  Receivers: right of NEAR and far from it (a), under the roof within 1 of the
    light (b), just right of NEAR (c); and rays that reach LIGHT_ON_FLOOR exactly, from several directions and distances (d)."""
    grid = lambda xs, zs: [(x, z) for x in xs for z in zs]
    recv = {"a": grid(np.linspace(3.5, 6.0, 6), np.linspace(5.2, 6.8, 5)),
            "b": grid(-2.0 + np.linspace(-0.4, 0.4, 5), 6.0 + np.linspace(-0.4, 0.4, 5)),
            "c": grid(np.linspace(1.3, 2.3, 6), np.linspace(5.2, 6.8, 5))}
    O = [(x, -2.6, z) for k in "abc" for x, z in recv[k]]
    D = [(0.0, -1.0, 0.0)] * len(O)
    for d in ((0, -1, 0), (1, -1, 0), (-1, -1, 0), (0, -1, 1), (0, -1, -1), (1, -1, 1)):
        for k in (0.5, 1.0, 2.0, 4.0):
            O.append(tuple(np.array(LIGHT_ON_FLOOR) - k * np.array(d, np.float64))); D.append(tuple(map(float, d)))
    return np.asarray(O, np.float64), np.asarray(D, np.float64)


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


class _Light:
    """What conftest.lights_tuple reads of a light, for the oracle alone (the CPU test does not load the product library)."""
    def __init__(self, kind, intensity, v):
        self.kind, self.intensity, self.v = kind, intensity, self
        self.x, self.y, self.z = v


def _lights(rrt, light):
    """Ambient + the one point light; rrt = None: for the oracle only."""
    if rrt is None:
        return [_Light(0, 0.25, (0.0, 0.0, 0.0)), _Light(1, 0.7, light)]
    return [rrt.Light.Ambient(0.25), rrt.Light.Point(0.7, rrt.Vector3d(*light))]


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
