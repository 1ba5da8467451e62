"""The hand-built scenes and light lists of the lighting tests (tests/test_gpu_lighting.py, tests/test_gpu_option_limits.py): a shadow box, a corridor of mirrors,
the shadow box with the corridor's oblique mirror in it, a 16-light list for the shadow box whose kept masks use every bit, and the scene, lights and rays of the
shadow-exit tests (tests/test_gpu_shadow_exit.py, tests/test_gpu_ray_queries.py).

Plain module, not a test module: pytest does not rewrite its asserts, so every assert here states both values in its message.  It holds no fixtures.
"""
import numpy as np

from gpu_checks import ROOT_BOX, PlainLight, checker, closed_box, flat_normals, quad


def _scene(rrt, groups, towards, materials, textures):
    """groups: [(triangles, material id)]; uv from x/z (or x/y) so that textures vary across every surface."""
    tris = [t for g, _ in groups for t in g]
    mat = np.array([m for g, m in groups for _ in g], np.uint32)
    assert len(mat) == 0 or int(mat.max()) < len(materials), f"material index {int(mat.max())} for a table of {len(materials)}"
    pos = np.asarray(tris, np.float64)
    uv = np.zeros_like(pos); uv[..., 0] = pos[..., 0] * 0.13 + pos[..., 2] * 0.07; uv[..., 1] = pos[..., 1] * 0.11 + pos[..., 2] * 0.05
    nrm = flat_normals(tris, towards)
    A = dict(pos=pos, uv=uv, nrm=nrm, mat=mat, materials=materials, textures=textures, root=ROOT_BOX)
    return rrt.SceneData.from_arrays(pos, uv, nrm, mat, materials, textures), A


SHADOW_ORIGIN = (0.0, 3.0, -10.0)
SHADOW_TOWARDS = (0.0, 3.0, 1.0)


def _shadow_box_parts():
    """(materials, textures, groups) of the shadow box"""
    mats = [dict(ka=(1, 1, 1), kd=(0.9, 0.9, 0.9), ks=(0.3, 0.3, 0.3), ns=20.0, kr=0.0, tex=0, bump=-1),
            dict(ka=(0.8, 0.8, 0.8), kd=(0.7, 0.7, 0.7), ks=(0.5, 0.5, 0.5), ns=60.0, kr=0.0, tex=1, bump=-1),
            dict(ka=(1, 1, 1), kd=(1, 1, 1), ks=(0, 0, 0), ns=-1.0, kr=0.0, tex=2, bump=-1)]
    tex = [checker((200, 180, 150), (90, 110, 140)), checker((150, 220, 120), (60, 60, 60), 4), np.full((2, 2, 3), 230, np.uint8)]
    groups = [(quad((-6, 0, -4), (6, 0, -4), (6, 0, 8), (-6, 0, 8)), 0),            # floor
              (quad((-6, 0, 8), (6, 0, 8), (6, 7, 8), (-6, 7, 8)), 1),              # back wall
              (quad((-6, 0, -4), (-6, 0, 8), (-6, 7, 8), (-6, 7, -4)), 1),          # left wall
              (quad((-1.5, 2, 0), (1.5, 2, 0), (1.5, 2, 2.5), (-1.5, 2, 2.5)), 2),  # blocker, 2 above the floor
              (closed_box((2, 0, 3), (4, 2, 5)), 1)]                                 # closed box
    return mats, tex, groups


def _shadow_box_scene(rrt):
    """Floor, back and left walls, a thin blocker 2 above the floor, and a closed box."""
    mats, tex, groups = _shadow_box_parts()
    return _scene(rrt, groups, SHADOW_TOWARDS, mats, tex)


# 16 lights for the shadow box, (kind, intensity, vector), kinds 0 = Ambient, 1 = Point, 2 = Directional.  Most point lights lie outside the hull of the walls on
# its open sides (right, front, above), so a shadow ray -- which runs to t = |L - p| in units of its unnormalised direction, far past the light -- leaves the scene
# instead of ending in the wall behind the light: both lit and dark points occur for every point light, and lit lights behind the first dark one.
SIXTEEN = ((0, 0.1, (0.0, 0.0, 0.0)), (1, 0.12, (-3.0, 9.0, -6.0)), (2, 0.05, (0.5, 1.0, -1.0)), (1, 0.08, (8.0, 6.0, -3.0)),
           (1, 0.1, (7.0, 8.0, -6.0)), (0, 0.05, (0.0, 0.0, 0.0)), (1, 0.07, (9.0, 1.0, 6.0)), (2, 0.05, (-1.0, 2.0, 0.5)),
           (1, 0.07, (8.0, 0.5, -2.0)), (1, 0.06, (0.0, 1.0, 1.2)), (0, 0.05, (0.0, 0.0, 0.0)), (1, 0.06, (3.0, 12.0, 4.0)),
           (1, 0.06, (-2.0, 10.0, -8.0)), (2, 0.04, (0.2, 1.0, -0.3)), (1, 0.06, (9.0, 3.0, 4.0)), (1, 0.08, (0.0, 9.0, 1.2)))
assert len(SIXTEEN) == 16, f"SIXTEEN holds {len(SIXTEEN)} lights"


def lights_of(rrt, triples):
    """The package's Light objects of (kind, intensity, vector) triples."""
    return [rrt.Light(int(k), float(i), rrt.Vector3d(*map(float, v))) for k, i, v in triples]


CORRIDOR_ORIGIN = (0.0, 1.0, -8.0)
OBLIQUE_MIRROR = quad((4, -3, -6), (9, -3, 0), (9, 6, 0), (4, 6, -6))                   # 50 degrees to the corridor's axis
OBLIQUE_MATERIAL = dict(ka=(1, 1, 1), kd=(0.7, 0.7, 0.7), ks=(0.2, 0.2, 0.2), ns=10.0, kr=0.6, tex=2, bump=-1)
OBLIQUE_TEXTURE = ((30, 240, 40), (90, 200, 20), 4)                                     # checker's arguments


def _corridor_scene(rrt):
    """Two facing mirrors (z = 8 and z = -12) with different kr and textures, an oblique mirror on the right and a floor."""
    mats = [dict(ka=(1, 1, 1), kd=(0.8, 0.8, 0.8), ks=(0.6, 0.6, 0.6), ns=40.0, kr=0.85, tex=0, bump=-1),
            dict(ka=(1, 1, 1), kd=(0.8, 0.8, 0.8), ks=(0.6, 0.6, 0.6), ns=40.0, kr=0.75, tex=1, bump=-1),
            dict(OBLIQUE_MATERIAL),
            dict(ka=(1, 1, 1), kd=(1, 1, 1), ks=(0, 0, 0), ns=-1.0, kr=0.0, tex=3, bump=-1)]
    tex = [checker((250, 40, 30), (200, 20, 60), 4), checker((20, 40, 250), (60, 20, 200), 4), checker(*OBLIQUE_TEXTURE),
           checker((180, 180, 180), (90, 90, 90))]
    groups = [(quad((-15, -10, 8), (15, -10, 8), (15, 10, 8), (-15, 10, 8)), 0),
              (quad((-15, -10, -12), (15, -10, -12), (15, 10, -12), (-15, 10, -12)), 1),
              (OBLIQUE_MIRROR, 2),
              (quad((-15, -3, -12), (15, -3, -12), (15, -3, 8), (-15, -3, 8)), 3)]       # floor
    return _scene(rrt, groups, (0.0, 1.0, -2.0), mats, tex)


def _corridor_lights(rrt):
    L, V = rrt.Light, rrt.Vector3d
    return [L.Ambient(0.3), L.Point(0.4, V(-5.0, 4.0, 4.0)), L.Point(0.4, V(5.0, 3.0, -9.0)), L.Directional(0.2, V(0.0, 1.0, -0.3))]


MIRROR_SHIFT = (-10.0, 3.0, 6.0)


def _shadow_box_mirror_scene(rrt):
    """The shadow box with the corridor's oblique mirror (kr 0.6) standing in it, moved by MIRROR_SHIFT across the closed back-left corner -- from the left wall at
    z = 0 to the back wall's foot at x = -1 -- where it faces the open sides and does not stand between the floor and the lights of SIXTEEN outside them."""
    mats, tex, groups = _shadow_box_parts()
    mats.append(dict(OBLIQUE_MATERIAL, tex=len(tex)))
    tex.append(checker(*OBLIQUE_TEXTURE))
    moved = (np.asarray(OBLIQUE_MIRROR, np.float64) + np.asarray(MIRROR_SHIFT)).tolist()
    groups.append((moved, len(mats) - 1))
    return _scene(rrt, groups, SHADOW_TOWARDS, mats, tex)


# ------------------------------------------------------------------ the scene of the shadow-exit tests (tests/test_gpu_shadow_exit.py describes its classes of rays)
SHADOW_EXIT_OFFSET = 1e-4                                # SURFACE_OFFSET, raytracer.rs:17
SHADOW_EXIT_LIGHT_ABOVE = (-2.0, -2.75, 6.0)             # classes (a), (b), (c): a quarter above the floor
SHADOW_EXIT_LIGHT_ON_FLOOR = (3.0, -3.0, 7.0)            # class (d): a point of the floor that rays hit exactly
SHADOW_EXIT_CAMERA = (0.0, 2.0, -10.0)


def shadow_exit_arrays():
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


def shadow_exit_rays():
    """Straight down onto the floor from y = -2.6 (under the roof).  Receivers: right of NEAR and far from it (a), under the roof within 1 of the
    light (b), just right of NEAR (c); and rays that reach SHADOW_EXIT_LIGHT_ON_FLOOR exactly, from several directions and distances (d)."""
    grid = lambda xs, zs: [(x, z) for x in xs for z in zs]
    recv = {"a": grid(np.linspace(3.5, 6.0, 6), np.linspace(5.2, 6.8, 5)),
            "b": grid(-2.0 + np.linspace(-0.4, 0.4, 5), 6.0 + np.linspace(-0.4, 0.4, 5)),
            "c": grid(np.linspace(1.3, 2.3, 6), np.linspace(5.2, 6.8, 5))}
    O = [(x, -2.6, z) for k in "abc" for x, z in recv[k]]
    D = [(0.0, -1.0, 0.0)] * len(O)
    for d in ((0, -1, 0), (1, -1, 0), (-1, -1, 0), (0, -1, 1), (0, -1, -1), (1, -1, 1)):
        for k in (0.5, 1.0, 2.0, 4.0):
            O.append(tuple(np.array(SHADOW_EXIT_LIGHT_ON_FLOOR) - k * np.array(d, np.float64))); D.append(tuple(map(float, d)))
    return np.asarray(O, np.float64), np.asarray(D, np.float64)


def shadow_exit_lights(rrt, light):
    """Ambient + the one point light; rrt = None: for the oracle only (what conftest.lights_tuple reads of a light, without loading the product library)."""
    if rrt is None:
        return [PlainLight(0, 0.25, (0.0, 0.0, 0.0)), PlainLight(1, 0.7, light)]
    return [rrt.Light.Ambient(0.25), rrt.Light.Point(0.7, rrt.Vector3d(*light))]
