"""The camera part of the C ABI that needs no GPU: struct layout, argument checks (made before any HIP call) and rrt_camera_look_at, which is host code."""
import ctypes as C

import numpy as np
import pytest

from scenes import TARGET

EYES = ((6, 3, -8), (-7, 4, -6), (9, 2, 1), (0, 9, -4), (4, 1.5, 7), (0, 2, -6))   # the poses of tests/test_gpu_camera.py


def test_camera_struct_is_96_bytes(rrt):
    assert C.sizeof(rrt.CCamera) == 96
    assert [n for n, _ in rrt.CCamera._fields_] == ["eye", "right", "up", "forward"]


def test_set_and_get_camera_refuse_a_null_raytracer(rrt):
    L = rrt.lib()
    cam = rrt.CCamera(rrt.Vec3(0, 0, 0), rrt.Vec3(1, 0, 0), rrt.Vec3(0, 1, 0), rrt.Vec3(0, 0, 1))
    assert L.rrt_raytracer_set_camera(None, C.byref(cam)) == rrt.ERR_INVALID_ARG
    assert L.rrt_raytracer_set_camera(None, None) == rrt.ERR_INVALID_ARG
    assert L.rrt_raytracer_get_camera(None, C.byref(cam)) == rrt.ERR_INVALID_ARG
    assert L.rrt_camera_look_at(rrt.Vec3(0, 0, 0), rrt.Vec3(0, 0, 1), rrt.Vec3(0, 1, 0), None) == rrt.ERR_INVALID_ARG


def test_look_at_from_the_reference_camera_is_the_identity_basis(rrt):
    """main.rs:62-66 looks from (0, 2, -10) down +z: look_at along that axis gives exactly the creation pose."""
    cam = rrt.look_at((0, 2, -10), (0, 2, 0))
    assert cam == {"eye": (0.0, 2.0, -10.0), "right": (1.0, 0.0, 0.0), "up": (0.0, 1.0, 0.0), "forward": (0.0, 0.0, 1.0)}
    assert rrt.look_at(rrt.Vector3d(0, 2, -10), rrt.Vector3d(0, 2, 0), rrt.Vector3d(0, 1, 0)) == cam


@pytest.mark.parametrize("eye", EYES)
def test_look_at_gives_an_orthonormal_left_handed_basis(rrt, eye):
    """Tolerance 8 eps (1.8e-15): a component of forward or right carries up to 3 roundings (subtraction, sqrt of the length, division), one of up or of a
    dot / cross product checked here up to 3 more, all on values of magnitude <= 1."""
    tol = 8 * np.finfo(np.float64).eps
    cam = rrt.look_at(eye, TARGET)
    r, u, f = (np.array(cam[k]) for k in ("right", "up", "forward"))
    assert cam["eye"] == tuple(map(float, eye))
    for a in (r, u, f):
        assert abs(np.dot(a, a) - 1.0) <= tol
    assert abs(np.dot(r, u)) <= tol and abs(np.dot(r, f)) <= tol and abs(np.dot(u, f)) <= tol
    d = np.array(TARGET) - np.array(eye, np.float64)
    assert np.abs(f - d / np.linalg.norm(d)).max() <= tol                     # forward along target - eye
    assert np.abs(np.cross(u, f) - r).max() <= tol                            # left-handed, x right / y up / z forward: up x forward = right ...
    assert np.abs(np.cross(f, r) - u).max() <= tol                            # ... forward x right = up (the identity basis satisfies both)
    assert u[1] > 0 and r[1] == 0.0                                           # up_hint = +y: up leans to +y, right is horizontal


def test_look_at_refuses_degenerate_input(rrt):
    nan, inf = float("nan"), float("inf")
    for eye, target, up in (((1, 2, 3), (1, 2, 3), (0, 1, 0)),                # target == eye
                            ((0, 0, 0), (0, 5, 0), (0, 1, 0)),                # up_hint parallel to the view direction
                            ((0, 0, 0), (0, -5, 0), (0, 3, 0)),               # ... anti-parallel
                            ((0, 0, 0), (0, 0, 5), (0, 0, 0)),                # zero up_hint
                            ((nan, 0, 0), (0, 0, 5), (0, 1, 0)), ((0, 0, 0), (0, nan, 5), (0, 1, 0)), ((0, 0, 0), (0, 0, 5), (0, 1, nan)),
                            ((0, 0, 0), (inf, 0, 5), (0, 1, 0))):
        with pytest.raises(rrt.RrtError) as e:
            rrt.look_at(eye, target, up)
        assert e.value.status == rrt.ERR_INVALID_ARG, (eye, target, up)
