"""The poses, frames and scene fixtures that more than one GPU test module uses, each defined here once.

Constants: the creation pose and the moved eyes, the 203 x 117 frame of the region tests with its eye and regions.  Functions: pose, posed, rays_of.
Fixtures (scope="module": every module that imports one builds its own): the teapot's arrays with and without the root box, the teapot's oracle scene, the
mirror room with and without its oracle scene, and the raytracer at EYE3 with its whole-frame planes in the three forms the surface, visibility and shade tests
keep.  A test module takes a fixture by importing the function by name (`# noqa: F401`), together with every fixture that one requests.

The scenes themselves are built where their feature's helpers live: gpu_checks.py (chain scenes, plane scenes), shade_checks.py (mirror room, soup),
lighting_scenes.py (shadow box, corridor, the shadow-exit scene).
"""
import numpy as np
import pytest

from gpu_checks import ORIGIN, ROOT_BOX, oracle_for
from shade_checks import MIRROR_ROOM_LIGHTS, mirror_room
from surface_checks import frame_dirs

IDENTITY = dict(right=(1.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), forward=(0.0, 0.0, 1.0))
CREATION = dict(eye=ORIGIN, **IDENTITY)
TARGET = (0.0, 1.0, 0.0)
MOVED_EYE = (9.0, 2.0, 1.0)

# the frame, the eye and the regions of the region tests (tests/test_gpu_surface.py part 4, tests/test_gpu_visibility.py part 3, tests/test_gpu_shade.py part 6)
W3, H3 = 203, 117
EYE3 = (-7.0, 4.0, -6.0)
REGIONS = ((0, 0, 203, 117), (5, 3, 1, 1), (200, 0, 3, 2), (8, 8, 8, 8), (13, 50, 77, 31))


def pose(rrt, k, eyes=(MOVED_EYE,)):
    """Pose 0 is the creation pose, pose k looks from eyes[k - 1] at TARGET."""
    return CREATION if k == 0 else rrt.look_at(eyes[k - 1], TARGET)


def posed(rt, cam):
    rt.set_camera(**cam)
    return rt


def rays_of(cam, w, h, viewport=(1.0, 1.0, 1.0)):
    """(origins, directions) of the traced sub-sample rays of a w x h frame in the pose `cam`, in the planes' index order."""
    d = frame_dirs(cam, w, h, viewport).reshape(-1, 3)
    return np.ascontiguousarray(np.broadcast_to(np.asarray(cam["eye"], np.float64), d.shape)), d


# ------------------------------------------------------------------ the teapot
def arrays_of(sd, root=None):
    """The arrays dict of a SceneData, as gpu_checks.oracle_for reads it; with root, the root box is stated in it."""
    pos, uv, nrm, mat = sd.triangles()
    return dict(pos=pos, uv=uv, nrm=nrm, mat=mat, materials=sd.materials(), textures=sd.textures(), **({} if root is None else {"root": root}))


@pytest.fixture(scope="module")
def teapot_arrays(teapot):
    return arrays_of(teapot)


@pytest.fixture(scope="module")
def teapot_arrays_with_root(teapot):
    return arrays_of(teapot, ROOT_BOX)


@pytest.fixture(scope="module")
def teapot_osc(ob, rrt, teapot_arrays):
    return oracle_for(ob, teapot_arrays, rrt.default_lights())


# ------------------------------------------------------------------ the mirror room
def mirror_room_scene(rrt):
    """(arrays, lights, SceneData) of shade_checks.mirror_room with MIRROR_ROOM_LIGHTS"""
    A = mirror_room()
    lights = [rrt.Light(k, i, rrt.Vector3d(*v)) for k, i, v in MIRROR_ROOM_LIGHTS]
    return A, lights, rrt.SceneData.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], A["materials"], A["textures"])


@pytest.fixture(scope="module")
def room(rrt, ob):
    """(arrays, lights, SceneData, oracle scene) of the mirror room"""
    A, lights, sd = mirror_room_scene(rrt)
    return A, lights, sd, oracle_for(ob, A, lights)


@pytest.fixture(scope="module")
def room_without_oracle(rrt):
    """(arrays, lights, SceneData) of the mirror room, for the modules that compare the library with itself"""
    return mirror_room_scene(rrt)


# ------------------------------------------------------------------ the raytracer at EYE3 and its whole-frame planes
def frame3_of(rrt, teapot, planes_of, render=False):
    """A raytracer at EYE3 that has rendered no frame before planes_of(rt) gave its whole-frame planes; with render, its frame after them.  Read-only."""
    rt = rrt.RayTracer(teapot, rrt.default_lights())
    rt.look_at(EYE3, TARGET)
    full = planes_of(rt)
    frame = rt.render(W3, H3) if render else None
    for a in list(full.values()) + ([frame] if render else []):
        a.setflags(write=False)
    return (rt, frame, full) if render else (rt, full)


@pytest.fixture(scope="module")
def surface_frame3(rrt, teapot):
    """(raytracer that has rendered no frame, its surface and visibility planes)"""
    return frame3_of(rrt, teapot, lambda rt: rt.surface(W3, H3, visibility=rrt.PLANES))


@pytest.fixture(scope="module")
def visibility_frame3(rrt, teapot):
    """(raytracer that has rendered no frame, its visibility planes)"""
    return frame3_of(rrt, teapot, lambda rt: rt.visibility(W3, H3))


@pytest.fixture(scope="module")
def shade_frame3(rrt, teapot):
    """(raytracer, its frame, its surface planes with the albedo)"""
    return frame3_of(rrt, teapot, lambda rt: rt.surface(W3, H3, visibility=("albedo",)), render=True)
