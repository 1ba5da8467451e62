"""ctypes binding of oracle/liboracle.so -- TEST INFRASTRUCTURE ONLY (see oracle/rrt_oracle.h).

Importers allowed: tests/, __graft_entry__.smoke(), bench.py's cpu_baseline leg.  The product package
(rust-ray-tracer_amd/) must never import this module.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liboracle.so")


class OVec3(C.Structure):
    _fields_ = [("x", C.c_double), ("y", C.c_double), ("z", C.c_double)]


class OLight(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("_pad", C.c_uint32), ("intensity", C.c_double), ("v", OVec3)]


class OMaterial(C.Structure):
    _fields_ = [("ka", OVec3), ("kd", OVec3), ("ks", OVec3), ("ns", C.c_double), ("kr", C.c_double), ("tex", C.c_int32), ("bump", C.c_int32)]


class OTexture(C.Structure):
    _fields_ = [("rgb", C.POINTER(C.c_uint8)), ("width", C.c_uint32), ("height", C.c_uint32)]


class OCounters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("rays_primary", "rays_shadow", "rays_reflect", "tri_tests", "aabb_tests", "nodes_entered", "hits_shaded")]


_dp, _u32p, _u8p, _P = C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.c_void_p
_lib = None


def build():
    subprocess.run(["make", "-C", _HERE, "-s"], check=True)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            build()
        L = C.CDLL(LIB_PATH)
        L.oracle_scene_create.restype = _P
        L.oracle_scene_create.argtypes = [C.c_uint32, _dp, _dp, _dp, _u32p, C.c_uint32, C.POINTER(OMaterial), C.c_uint32, C.POINTER(OTexture),
                                          C.c_uint32, C.POINTER(OLight), OVec3, _dp]
        L.oracle_scene_destroy.argtypes = [_P]; L.oracle_scene_destroy.restype = None
        L.oracle_scene_set_options.argtypes = [_P, C.c_double, C.c_uint32]; L.oracle_scene_set_options.restype = None
        L.oracle_octree_num_nodes.argtypes = [_P]; L.oracle_octree_num_nodes.restype = C.c_uint32
        L.oracle_octree_max_depth.argtypes = [_P]; L.oracle_octree_max_depth.restype = C.c_uint32
        L.oracle_octree_own_total.argtypes = [_P]; L.oracle_octree_own_total.restype = C.c_uint32
        L.oracle_octree_export.argtypes = [_P, _dp, _u32p, _u32p, _u32p, _u32p]; L.oracle_octree_export.restype = None
        L.oracle_intersect_aabb.argtypes = [OVec3, OVec3, _dp, _dp]; L.oracle_intersect_aabb.restype = C.c_int
        L.oracle_intersect_triangle.argtypes = [OVec3, OVec3, _dp, _dp, _dp, _dp]; L.oracle_intersect_triangle.restype = C.c_int
        L.oracle_intersect_scene.argtypes = [_P, OVec3, OVec3, C.c_double, _dp, _dp, _dp, _u32p]; L.oracle_intersect_scene.restype = C.c_int
        L.oracle_get_ray_colour.argtypes = [_P, OVec3, OVec3]; L.oracle_get_ray_colour.restype = C.c_uint32
        L.oracle_color_mix4.argtypes = [C.c_uint32] * 4; L.oracle_color_mix4.restype = C.c_uint32
        L.oracle_f64_as_usize.argtypes = [C.c_double]; L.oracle_f64_as_usize.restype = C.c_uint64
        L.oracle_clamp_u8.argtypes = [C.c_double]; L.oracle_clamp_u8.restype = C.c_uint8
        L.oracle_render.argtypes = [_P, C.c_uint32, C.c_uint32, _dp, C.c_uint32, _u32p, C.POINTER(OCounters)]; L.oracle_render.restype = C.c_int
        _lib = L
    return _lib


def _d(a):
    return a.ctypes.data_as(_dp)


def _v(p):
    return OVec3(float(p[0]), float(p[1]), float(p[2]))


class OracleScene:
    """pos/uv/nrm [n,3,3] f64, mat [n] u32, materials: dicts (ka,kd,ks,ns,kr,tex,bump), textures: [h,w,3] u8 arrays,
    lights: (kind, intensity, (x,y,z)), origin (x,y,z), root (min_x,max_x,min_y,max_y,min_z,max_z).
    surface_offset / max_reflection_depth: the RayTracer options (raytracer.rs:17, :20); the defaults are the reference's constants."""

    def __init__(self, pos, uv, nrm, mat, materials, textures, lights, origin, root=(-20.0, 20.0, -20.0, 20.0, -20.0, 20.0),
                 surface_offset=1e-4, max_reflection_depth=5):
        L = lib()
        pos = np.ascontiguousarray(pos, np.float64).reshape(-1, 9); uv = np.ascontiguousarray(uv, np.float64).reshape(-1, 9)
        nrm = np.ascontiguousarray(nrm, np.float64).reshape(-1, 9); mat = np.ascontiguousarray(mat, np.uint32)
        self._tex_keep = [np.ascontiguousarray(t, np.uint8) for t in textures]
        cm = (OMaterial * max(1, len(materials)))()
        for i, m in enumerate(materials):
            cm[i] = OMaterial(_v(m["ka"]), _v(m["kd"]), _v(m["ks"]), float(m["ns"]), float(m["kr"]), int(m["tex"]), int(m.get("bump", -1)))
        ct = (OTexture * max(1, len(self._tex_keep)))()
        for i, t in enumerate(self._tex_keep):
            ct[i] = OTexture(t.ctypes.data_as(_u8p), t.shape[1], t.shape[0])
        cl = (OLight * max(1, len(lights)))()
        for i, (kind, inten, v) in enumerate(lights):
            cl[i] = OLight(int(kind), 0, float(inten), _v(v))
        r = np.asarray(root, np.float64)
        self.n_tris = pos.shape[0]
        self._h = _P(L.oracle_scene_create(pos.shape[0], _d(pos), _d(uv), _d(nrm), mat.ctypes.data_as(_u32p), len(materials), cm,
                                           len(self._tex_keep), ct, len(lights), cl, _v(origin), _d(r)))
        if surface_offset != 1e-4 or max_reflection_depth != 5:
            L.oracle_scene_set_options(self._h, float(surface_offset), int(max_reflection_depth))
        self.origin = tuple(map(float, origin))

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None:
            _lib.oracle_scene_destroy(h)

    def octree(self) -> dict:
        L = lib()
        n = L.oracle_octree_num_nodes(self._h)
        aabb = np.empty((n, 6)); fc = np.empty(n, np.uint32); tc = np.empty(n, np.uint32); off = np.empty(n + 1, np.uint32)
        idx = np.empty(L.oracle_octree_own_total(self._h), np.uint32)
        u = lambda a: a.ctypes.data_as(_u32p)
        L.oracle_octree_export(self._h, _d(aabb), u(fc), u(tc), u(off), u(idx))
        return dict(aabb=aabb, first_child=fc, tri_count=tc, own_off=off, own_idx=idx, max_depth=L.oracle_octree_max_depth(self._h))

    def intersect(self, o, d, max_t=float("inf")):
        t = C.c_double(); u = C.c_double(); v = C.c_double(); tri = C.c_uint32()
        hit = lib().oracle_intersect_scene(self._h, _v(o), _v(d), float(max_t), C.byref(t), C.byref(u), C.byref(v), C.byref(tri))
        return (True, t.value, u.value, v.value, tri.value) if hit else (False, 0.0, 0.0, 0.0, 0xFFFFFFFF)

    def get_ray_colour(self, o, d) -> int:
        return int(lib().oracle_get_ray_colour(self._h, _v(o), _v(d)))

    def render(self, width, height, viewport=(1.0, 1.0, 1.0), n_threads=None):
        fb = np.empty((height, width), np.uint32)
        cnt = OCounters()
        vp = np.asarray(viewport, np.float64)
        lib().oracle_render(self._h, width, height, _d(vp), n_threads or (os.cpu_count() or 1), fb.ctypes.data_as(_u32p), C.byref(cnt))
        return fb, {n: getattr(cnt, n) for n, _ in OCounters._fields_}


def intersect_aabb(o, d, box):
    b = np.asarray(box, np.float64); t = C.c_double()
    return (True, t.value) if lib().oracle_intersect_aabb(_v(o), _v(d), _d(b), C.byref(t)) else (False, None)


def intersect_triangle(o, d, verts):
    v9 = np.ascontiguousarray(verts, np.float64).reshape(9); t = C.c_double(); u = C.c_double(); v = C.c_double()
    return (True, t.value, u.value, v.value) if lib().oracle_intersect_triangle(_v(o), _v(d), _d(v9), C.byref(t), C.byref(u), C.byref(v)) else (False, None, None, None)
