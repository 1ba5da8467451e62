"""MI355X-native per-pixel hot path of conor722/rust-ray-tracer -- Python host mirror over the C ABI (include/rrt.h).

The names follow the reference's host code so tests read like the reference would test itself:

    SceneData  <- parse_obj_file_lines()          src/file_management/utils.rs:139, src/scene/scenedata.rs:5-13
    Light.*                                       src/scene/entities.rs:5-9
    RayTracer(scene_data, lights, origin)         src/scene/raytracer.rs:22-26   (.get_ray_colour -> raytracer.rs:29)
    Scene(width, height).draw_scene(rt)           src/scene/engine.rs:177,186    (fills scene.canvas.buffer, engine.rs:127)

Everything that computes goes through librrt_hip.so (hand-written HIP kernels, gfx950).  There is no CPU or
PyTorch fallback: if the library is missing, or no GPU is visible when a RayTracer is created, this raises.
PyTorch is only plumbing (device buffers, streams, torch.distributed) in `render_into` / `render_tiles_into`.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Iterable, Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RRT_LIB") or os.path.join(_HERE, "librrt_hip.so")   # RRT_LIB: developer override (e.g. the counters build)


class RrtError(RuntimeError):
    def __init__(self, status: int, what: str, detail: str):
        super().__init__(f"{what}: {detail or '?'} (status {status})")
        self.status = status
        self.detail = detail


FLAG_NO_CULL, FLAG_LANE_FILTER, FLAG_BUNDLE_FILTER, FLAG_RAY_WALK, FLAG_HOST_SETUP, FLAG_NO_CHAIN_SHORTCUT = 1, 2, 4, 8, 16, 32   # RRT_FLAG_*, include/rrt.h
BUFFERS = ("nodes", "geom", "attr", "supers", "cboxes", "child_boxes", "tboxes", "suspects", "oct_box", "oct_first_child", "oct_tri_count", "oct_own_off",
           "oct_own_idx", "slot_tri", "slot_pos", "chains")   # RRT_BUF_*
VARIANT_NAMES = ("lane", "bundle", "ray")   # rrt_stats.filter_variant

# status codes, include/rrt.h
OK, ERR_INVALID_ARG, ERR_HIP, ERR_OOM, ERR_IO, ERR_PARSE, ERR_DEPTH, ERR_NO_DEVICE, ERR_UNSUPPORTED = 0, -1, -2, -3, -4, -5, -6, -7, -8


class Vec3(C.Structure):
    _fields_ = [("x", C.c_double), ("y", C.c_double), ("z", C.c_double)]


class CLight(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("_pad", C.c_uint32), ("intensity", C.c_double), ("v", Vec3)]


class CMaterial(C.Structure):
    _fields_ = [("ka", Vec3), ("kd", Vec3), ("ks", Vec3), ("ns", C.c_double), ("kr", C.c_double), ("tex", C.c_int32), ("bump", C.c_int32)]


class CTexture(C.Structure):
    _fields_ = [("rgb", C.POINTER(C.c_uint8)), ("width", C.c_uint32), ("height", C.c_uint32)]


class COptions(C.Structure):
    _fields_ = [("surface_offset", C.c_double), ("max_reflection_depth", C.c_uint32), ("flags", C.c_uint32),
                ("vp_w", C.c_double), ("vp_h", C.c_double), ("vp_d", C.c_double)]


class CCamera(C.Structure):          # rrt_camera, 96 bytes
    _fields_ = [("eye", Vec3), ("right", Vec3), ("up", Vec3), ("forward", Vec3)]


class CRegion(C.Structure):          # rrt_region, 16 bytes
    _fields_ = [(n, C.c_uint32) for n in ("x0", "y0", "w", "h")]


class CVisibility(C.Structure):      # rrt_visibility, 48 bytes: host or device pointers, NULL = plane not wanted
    _fields_ = [(n, C.c_void_p) for n in ("hit", "t", "u", "v", "tri", "albedo")]


class CPickResult(C.Structure):      # rrt_pick_result, 40 bytes
    _fields_ = [("hit", C.c_uint32), ("tri", C.c_uint32), ("t", C.c_double), ("u", C.c_double), ("v", C.c_double), ("albedo", C.c_uint32), ("_pad", C.c_uint32)]


PLANES = ("hit", "t", "u", "v", "tri", "albedo")   # the planes of rrt_visibility, in its order
PLANE_DTYPES = dict(hit=np.uint8, t=np.float64, u=np.float64, v=np.float64, tri=np.uint32, albedo=np.uint32)


class CSurface(C.Structure):         # rrt_surface, 32 bytes: host or device pointers, NULL = plane not wanted
    _fields_ = [(n, C.c_void_p) for n in ("point", "normal", "material", "lights")]


SURFACE_PLANES = ("point", "normal", "material", "lights")   # the planes of rrt_surface, in its order
SURFACE_DTYPES = dict(point=np.float64, normal=np.float64, material=np.uint32, lights=np.uint32)
SURFACE_WIDTHS = dict(point=3, normal=3, material=1, lights=1)   # elements per sub-sample


class CAmbientSamples(C.Structure):  # rrt_ambient_samples, 24 bytes: dirs = n x 3 host doubles in the tangent frame of a hit
    _fields_ = [("dirs", C.POINTER(C.c_double)), ("n", C.c_uint32), ("_pad", C.c_uint32), ("max_t", C.c_double)]


class CAmbient(C.Structure):         # rrt_ambient, 16 bytes: host or device pointers, NULL = plane not wanted
    _fields_ = [(n, C.c_void_p) for n in ("occluded", "grey")]


MAX_AMBIENT_SAMPLES = 32             # RRT_MAX_AMBIENT_SAMPLES
AMBIENT_OUTPUTS = ("occluded", "grey")   # the planes of rrt_ambient, in its order: [h][w][4] masks, [h][w] pixels, both uint32


class CModelInfo(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("n_tris", "n_tris_in_tree", "n_nodes", "max_depth", "n_mats", "n_tex", "root_own_count", "max_own_count")]


class CStats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("width", C.c_uint32), ("height", C.c_uint32), ("rays_primary", C.c_uint64), ("scene_bytes", C.c_uint64),
                ("filter_variant", C.c_uint32), ("origin_plane_triangles", C.c_uint32),
                ("filter_pad", C.c_double), ("filter_alpha_unit", C.c_double), ("filter_delta_unit", C.c_double)]


class CSetupTimes(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("read_ms", "parse_ms", "texture_ms", "octree_ms", "index_ms", "upload_ms", "hip_init_ms", "create_ms", "gpu_setup")]


# every symbol include/rrt.h declares: (restype, argtypes)
_P = C.c_void_p
_dp, _u32p, _u8p = C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
SYMBOLS = {
    "rrt_model_load_obj": (C.c_int, [C.c_char_p, _dp, C.POINTER(_P)]),
    "rrt_model_from_arrays": (C.c_int, [C.c_uint32, _dp, _dp, _dp, _u32p, C.c_uint32, C.POINTER(CMaterial), C.c_uint32, C.POINTER(CTexture), _dp, C.POINTER(_P)]),
    "rrt_model_destroy": (None, [_P]),
    "rrt_model_get_info": (C.c_int, [_P, C.POINTER(CModelInfo)]),
    "rrt_model_get_triangles": (C.c_int, [_P, _dp, _dp, _dp, _u32p]),
    "rrt_model_get_materials": (C.c_int, [_P, C.POINTER(CMaterial)]),
    "rrt_model_get_texture": (C.c_int, [_P, C.c_uint32, C.POINTER(CTexture)]),
    "rrt_model_get_octree": (C.c_int, [_P, _dp, _u32p, _u32p, _u32p, _u32p]),
    "rrt_decode_image_file": (C.c_int, [C.c_char_p, C.POINTER(_u8p), _u32p, _u32p]),
    "rrt_free": (None, [_P]),
    "rrt_raytracer_create": (C.c_int, [_P, C.POINTER(CLight), C.c_uint32, Vec3, C.POINTER(COptions), C.c_int, C.POINTER(_P)]),
    "rrt_raytracer_create_from_arrays": (C.c_int, [C.c_uint32, _dp, _dp, _dp, _u32p, C.c_uint32, C.POINTER(CMaterial), C.c_uint32, C.POINTER(CTexture), _dp,
                                                  C.POINTER(CLight), C.c_uint32, Vec3, C.POINTER(COptions), C.c_int, C.POINTER(_P)]),
    "rrt_raytracer_destroy": (None, [_P]),
    "rrt_raytracer_set_camera": (C.c_int, [_P, C.POINTER(CCamera)]),
    "rrt_raytracer_get_camera": (C.c_int, [_P, C.POINTER(CCamera)]),
    "rrt_camera_look_at": (C.c_int, [Vec3, Vec3, Vec3, C.POINTER(CCamera)]),
    "rrt_raytracer_set_lights": (C.c_int, [_P, C.POINTER(CLight), C.c_uint32]),
    "rrt_raytracer_get_lights": (C.c_int, [_P, C.POINTER(CLight), C.c_uint32, _u32p]),
    "rrt_raytracer_set_materials": (C.c_int, [_P, C.POINTER(CMaterial), C.c_uint32]),
    "rrt_raytracer_get_materials": (C.c_int, [_P, C.POINTER(CMaterial), C.c_uint32, _u32p]),
    "rrt_raytracer_set_triangles": (C.c_int, [_P, C.c_uint32, _dp, _dp, _dp, _u32p, _dp]),
    "rrt_raytracer_set_triangles_device": (C.c_int, [_P, C.c_uint32, _P, _P, _P, _P, _dp, _P]),
    "rrt_raytracer_release_update_memory": (C.c_int, [_P]),
    "rrt_render": (C.c_int, [_P, C.c_uint32, C.c_uint32, _u32p]),
    "rrt_host_buffer_register": (C.c_int, [_P, C.c_size_t]),
    "rrt_host_buffer_unregister": (C.c_int, [_P]),
    "rrt_render_device": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P, _P]),
    "rrt_render_visibility_device": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.POINTER(CRegion), C.POINTER(CVisibility), _P]),
    "rrt_render_visibility": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.POINTER(CRegion), C.POINTER(CVisibility)]),
    "rrt_render_surface_device": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.POINTER(CRegion), C.POINTER(CVisibility), C.POINTER(CSurface), _P]),
    "rrt_render_surface": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.POINTER(CRegion), C.POINTER(CVisibility), C.POINTER(CSurface)]),
    "rrt_shade_surface_device": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.POINTER(CRegion), C.POINTER(CVisibility), C.POINTER(CSurface), _P, _P]),
    "rrt_shade_surface": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.POINTER(CRegion), C.POINTER(CVisibility), C.POINTER(CSurface), _u32p]),
    "rrt_ambient_surface_device": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.POINTER(CRegion), C.POINTER(CSurface), C.POINTER(CAmbientSamples), C.POINTER(CAmbient), _P]),
    "rrt_ambient_surface": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.POINTER(CRegion), C.POINTER(CSurface), C.POINTER(CAmbientSamples), C.POINTER(CAmbient)]),
    "rrt_pick": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(CPickResult)]),
    "rrt_tiles_per_rank": (C.c_uint32, [C.c_uint32, C.c_uint32, C.c_uint32]),
    "rrt_render_tiles_device": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _P, _P]),
    "rrt_detile_device": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint32, _P, _P, _P]),
    "rrt_multi_create": (C.c_int, [C.POINTER(_P), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(_P)]),
    "rrt_dist_unique_id": (C.c_int, [_P]),
    "rrt_dist_create": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P, C.c_uint32, C.POINTER(_P)]),
    "rrt_multi_destroy": (None, [_P]),
    "rrt_multi_enqueue": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P]),
    "rrt_multi_sync": (C.c_int, [_P]),
    "rrt_render_multi": (C.c_int, [_P, C.c_uint32, C.c_uint32, _u32p]),
    "rrt_multi_last_gather_ms": (C.c_int, [_P, _dp]),
    "rrt_render_progressive": (C.c_int, [_P, C.c_uint32, C.c_uint32, _u32p, C.c_uint32, _P, _P]),
    "rrt_get_ray_colours": (C.c_int, [_P, C.c_uint32, _dp, _dp, _u32p]),
    "rrt_intersect_rays": (C.c_int, [_P, C.c_uint32, _dp, _dp, _dp, _u8p, _dp, _dp, _dp, _u32p]),
    "rrt_occluded_rays": (C.c_int, [_P, C.c_uint32, _dp, _dp, _dp, _u8p]),
    "rrt_intersect_rays_device": (C.c_int, [_P, C.c_uint32, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "rrt_get_ray_colours_device": (C.c_int, [_P, C.c_uint32, _P, _P, _P, _P]),
    "rrt_occluded_rays_device": (C.c_int, [_P, C.c_uint32, _P, _P, _P, _P, _P]),
    "rrt_tune_rays_device": (C.c_int, [_P, C.c_uint32, _P, _P, _P, _u32p]),
    "rrt_raytracer_get_octree": (C.c_int, [_P, C.POINTER(CModelInfo), _dp, _u32p, _u32p, _u32p, _u32p]),
    "rrt_raytracer_get_buffer": (C.c_int, [_P, C.c_uint32, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "rrt_raytracer_get_chain_info": (C.c_int, [_P, _u32p, _u32p]),
    "rrt_last_stats": (C.c_int, [_P, C.POINTER(CStats)]),
    "rrt_get_setup_times": (C.c_int, [_P, _P, C.POINTER(CSetupTimes)]),
    "rrt_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "rrt_strerror": (C.c_char_p, [C.c_int]),
    "rrt_last_error_detail": (C.c_char_p, []),
    "rrt_build_info": (C.c_char_p, []),
}

_lib = None


def lib() -> C.CDLL:
    """Load librrt_hip.so (built by __graft_entry__.build() / csrc/Makefile).  Fails loudly when it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: the HIP extension was not built (run `python -c 'import __graft_entry__ as g; g.build()'`). "
                              "There is no CPU fallback.")
        # One HIP runtime per process.  The PyTorch wheel bundles its own libamdhip64.so (soname libamdhip64.so.7, the name this library needs), so
        # whichever is loaded FIRST serves both; loaded second, torch would bring up a second runtime by file path and find "No HIP GPUs".  Tests and
        # bench.py use torch for device buffers, so it goes first here (RRT_NO_TORCH_PRELOAD=1: a host without torch in the process).
        if os.environ.get("RRT_NO_TORCH_PRELOAD") != "1":
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


def _check(status: int, what: str):
    if status != OK:
        L = lib()
        detail = (L.rrt_last_error_detail() or b"").decode(errors="replace")
        raise RrtError(status, f"{what} failed [{L.rrt_strerror(status).decode()}]", detail)


def _d(a: np.ndarray):
    return a.ctypes.data_as(_dp)


def device_count() -> int:
    n = C.c_int(0)
    _check(lib().rrt_device_count(C.byref(n)), "rrt_device_count")
    return n.value


# ---------------------------------------------------------------------------------------------- reference-shaped host types
@dataclass
class Vector3d:                      # src/scene/engine.rs:9-14
    x: float
    y: float
    z: float

    def _c(self) -> Vec3:
        return Vec3(float(self.x), float(self.y), float(self.z))


@dataclass
class Light:                         # src/scene/entities.rs:5-9
    kind: int
    intensity: float
    v: Vector3d

    @staticmethod
    def Ambient(intensity: float) -> "Light":
        return Light(0, intensity, Vector3d(0.0, 0.0, 0.0))

    @staticmethod
    def Point(intensity: float, position: Vector3d) -> "Light":
        return Light(1, intensity, position)

    @staticmethod
    def Directional(intensity: float, direction: Vector3d) -> "Light":
        return Light(2, intensity, direction)


def default_lights() -> list:
    """The lights `main` hard-codes, in its order (src/main.rs:32-58)."""
    return [Light.Ambient(0.5), Light.Point(0.4, Vector3d(-7.0, 1.0, -15.0)), Light.Point(0.5, Vector3d(0.0, 1.0, -41.0)),
            Light.Directional(0.4, Vector3d(-5.0, 0.0, 20.0))]


DEFAULT_ORIGIN = Vector3d(0.0, 2.0, -10.0)   # src/main.rs:62-66
DEFAULT_ROOT = (-20.0, 20.0, -20.0, 20.0, -20.0, 20.0)   # src/file_management/utils.rs:145


def _vec3(v) -> Vec3:
    """A Vector3d or any three numbers."""
    return v._c() if isinstance(v, Vector3d) else Vec3(*map(float, v))


def _camera_dict(c: CCamera) -> dict:
    return {n: (getattr(c, n).x, getattr(c, n).y, getattr(c, n).z) for n, _ in CCamera._fields_}


def look_at(eye, target, up=(0.0, 1.0, 0.0)) -> dict:
    """rrt_camera_look_at (host only): the pose at `eye` looking at `target`, left-handed like the reference (x right, y up, z forward), as a dict
    eye / right / up / forward of 3-tuples -- RayTracer.set_camera(**look_at(...)) applies it."""
    c = CCamera()
    _check(lib().rrt_camera_look_at(_vec3(eye), _vec3(target), _vec3(up), C.byref(c)), "rrt_camera_look_at")
    return _camera_dict(c)


class _Arrays:
    pass


def _marshal_arrays(pos, uv, nrm, mat, materials, textures, root):
    """ctypes views of a scene held in numpy arrays (no copies of arrays that are already contiguous float64 / uint32 / uint8)."""
    a = _Arrays()
    a.pos = np.ascontiguousarray(pos, np.float64).reshape(-1, 9)
    a.uv = np.ascontiguousarray(uv, np.float64).reshape(-1, 9)
    a.nrm = np.ascontiguousarray(nrm, np.float64).reshape(-1, 9)
    a.mat = np.ascontiguousarray(mat, np.uint32)
    a.n = a.pos.shape[0]
    a.cm = (CMaterial * max(1, len(materials)))()
    for i, m in enumerate(materials):
        a.cm[i] = CMaterial(Vec3(*m["ka"]), Vec3(*m["kd"]), Vec3(*m["ks"]), float(m["ns"]), float(m["kr"]), int(m["tex"]), int(m.get("bump", -1)))
    a.keep = [np.ascontiguousarray(t, np.uint8) for t in textures]
    a.ct = (CTexture * max(1, len(a.keep)))()
    for i, t in enumerate(a.keep):
        a.ct[i] = CTexture(t.ctypes.data_as(_u8p), t.shape[1], t.shape[0])
    a.r = (C.c_double * 6)(*root)
    return a


class SceneData:
    """SceneData (scenedata.rs:5-13): triangles in push order + materials + decoded textures + the octree."""

    def __init__(self, handle: int):
        self._h = _P(handle)
        self._info = None

    @property
    def info(self) -> dict:
        """rrt_model_get_info.  Builds the HOST copy of the octree on first use (the default GPU set-up of a RayTracer never needs it), so this is
        also where a too-deep tree (RRT_ERR_DEPTH) is reported on the host side."""
        if self._info is None:
            info = CModelInfo()
            _check(lib().rrt_model_get_info(self._h, C.byref(info)), "rrt_model_get_info")
            self._info = {n: getattr(info, n) for n, _ in CModelInfo._fields_}
        return self._info

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None:
            _lib.rrt_model_destroy(h)

    @staticmethod
    def from_arrays(pos, uv, nrm, mat, materials: Sequence[dict], textures: Sequence[np.ndarray], root=DEFAULT_ROOT) -> "SceneData":
        """pos/uv/nrm: [n,3,3] float64; mat: [n] uint32; materials: dicts ka,kd,ks,ns,kr,tex,bump; textures: [h,w,3] uint8."""
        a = _marshal_arrays(pos, uv, nrm, mat, materials, textures, root)
        out = _P()
        _check(lib().rrt_model_from_arrays(a.n, _d(a.pos), _d(a.uv), _d(a.nrm), a.mat.ctypes.data_as(_u32p), len(materials), a.cm, len(a.keep), a.ct, a.r, C.byref(out)),
               "rrt_model_from_arrays")
        return SceneData(out.value)

    # --- accessors
    def triangles(self):
        n = self.info["n_tris"]
        pos, uv, nrm, mat = (np.empty((n, 3, 3)), np.empty((n, 3, 3)), np.empty((n, 3, 3)), np.empty(n, np.uint32))
        _check(lib().rrt_model_get_triangles(self._h, _d(pos), _d(uv), _d(nrm), mat.ctypes.data_as(_u32p)), "rrt_model_get_triangles")
        return pos, uv, nrm, mat

    def materials(self) -> list:
        n = self.info["n_mats"]
        cm = (CMaterial * max(1, n))()
        _check(lib().rrt_model_get_materials(self._h, cm), "rrt_model_get_materials")
        v = lambda a: (a.x, a.y, a.z)
        return [dict(ka=v(m.ka), kd=v(m.kd), ks=v(m.ks), ns=m.ns, kr=m.kr, tex=m.tex, bump=m.bump) for m in cm[:n]]

    def texture(self, i: int) -> np.ndarray:
        t = CTexture()
        _check(lib().rrt_model_get_texture(self._h, i, C.byref(t)), "rrt_model_get_texture")
        return np.ctypeslib.as_array(t.rgb, shape=(t.height, t.width, 3)).copy()

    def textures(self) -> list:
        return [self.texture(i) for i in range(self.info["n_tex"])]

    def octree(self) -> dict:
        n = self.info["n_nodes"]
        aabb = np.empty((n, 6)); fc = np.empty(n, np.uint32); tc = np.empty(n, np.uint32); off = np.empty(n + 1, np.uint32)
        idx = np.empty(self.info["n_tris_in_tree"], np.uint32)
        u = lambda a: a.ctypes.data_as(_u32p)
        _check(lib().rrt_model_get_octree(self._h, _d(aabb), u(fc), u(tc), u(off), u(idx)), "rrt_model_get_octree")
        return dict(aabb=aabb, first_child=fc, tri_count=tc, own_off=off, own_idx=idx, max_depth=self.info["max_depth"])


def parse_obj_file(path: str, root=DEFAULT_ROOT) -> SceneData:
    """fs::read_to_string + parse_obj_file_lines (src/main.rs:28-30, src/file_management/utils.rs:139-213)."""
    r = (C.c_double * 6)(*root)
    out = _P()
    _check(lib().rrt_model_load_obj(os.fsencode(path), r, C.byref(out)), f"parse_obj_file({path})")
    return SceneData(out.value)


def decode_image_file(path: str) -> np.ndarray:
    """The build-owned stand-in for `image::ImageReader::open(..).decode()` (utils.rs:345-350): [h,w,3] uint8."""
    p = _u8p(); w = C.c_uint32(); h = C.c_uint32()
    _check(lib().rrt_decode_image_file(os.fsencode(path), C.byref(p), C.byref(w), C.byref(h)), f"decode_image_file({path})")
    try:
        return np.ctypeslib.as_array(p, shape=(h.value, w.value, 3)).copy()
    finally:
        lib().rrt_free(p)


class RayTracer:
    """RayTracer{scene_data, lights, origin} (raytracer.rs:22-26), uploaded once to one MI355X."""

    def __init__(self, scene_data: SceneData, lights: Iterable[Light], origin: Vector3d = DEFAULT_ORIGIN, device: int = 0,
                 surface_offset: float = 0.0001, max_reflection_depth: int = 5, viewport=(1.0, 1.0, 1.0), no_cull: bool = False,
                 box_filter: Optional[str] = None, host_setup: bool = False, chain_shortcut: bool = True):
        """no_cull=True (RRT_FLAG_NO_CULL): walk every own list in full, in list order, as ray.rs:119-129; default uses the cluster boxes.
        box_filter: None = rule of thumb on the first frame of a size, measured on the second, "lane" / "bundle" / "ray" = forced (RRT_FLAG_LANE_FILTER / RRT_FLAG_BUNDLE_FILTER /
        RRT_FLAG_RAY_WALK); same pixels.  host_setup=True (RRT_FLAG_HOST_SETUP): octree, index and records built on the host and uploaded (default: built on
        the GPU, csrc/scene_build.hip); same bytes in HBM.  chain_shortcut=False (RRT_FLAG_NO_CHAIN_SHORTCUT): the bundle-filter walk enters every node of a
        one-child chain; same results."""
        self.scene_data, self.origin, self.device = scene_data, origin, device
        lights = list(lights)                                  # (not kept: lights() asks the library for the list in force)
        cl = (CLight * max(1, len(lights)))()
        for i, l in enumerate(lights):
            cl[i] = CLight(l.kind, 0, float(l.intensity), l.v._c())
        flags = (FLAG_NO_CULL if no_cull else 0) | (FLAG_HOST_SETUP if host_setup else 0) | (0 if chain_shortcut else FLAG_NO_CHAIN_SHORTCUT) | {None: 0, "lane": FLAG_LANE_FILTER, "bundle": FLAG_BUNDLE_FILTER, "ray": FLAG_RAY_WALK}[box_filter]
        opt = COptions(surface_offset, max_reflection_depth, flags, *map(float, viewport))
        out = _P()
        _check(lib().rrt_raytracer_create(scene_data._h, cl, len(lights), origin._c(), C.byref(opt), device, C.byref(out)), "rrt_raytracer_create")
        self._h = out

    @classmethod
    def from_arrays(cls, pos, uv, nrm, mat, materials: Sequence[dict], textures: Sequence[np.ndarray], lights: Iterable[Light], origin: Vector3d = DEFAULT_ORIGIN,
                    device: int = 0, root=DEFAULT_ROOT, no_cull: bool = False, box_filter: Optional[str] = None) -> "RayTracer":
        """rrt_raytracer_create_from_arrays: the raytracer straight from the host's arrays (no SceneData / rrt_model, no host copy of the scene)."""
        self = cls.__new__(cls)
        self.scene_data, self.origin, self.device = None, origin, device
        lights = list(lights)
        a = _marshal_arrays(pos, uv, nrm, mat, materials, textures, root)
        cl = (CLight * max(1, len(lights)))()
        for i, l in enumerate(lights):
            cl[i] = CLight(l.kind, 0, float(l.intensity), l.v._c())
        flags = (FLAG_NO_CULL if no_cull else 0) | {None: 0, "lane": FLAG_LANE_FILTER, "bundle": FLAG_BUNDLE_FILTER, "ray": FLAG_RAY_WALK}[box_filter]
        opt = COptions(0.0001, 5, flags, 1.0, 1.0, 1.0)
        out = _P()
        _check(lib().rrt_raytracer_create_from_arrays(a.n, _d(a.pos), _d(a.uv), _d(a.nrm), a.mat.ctypes.data_as(_u32p), len(materials), a.cm, len(a.keep), a.ct, a.r,
                                                      cl, len(lights), origin._c(), C.byref(opt), device, C.byref(out)), "rrt_raytracer_create_from_arrays")
        self._h = out
        return self

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None:
            _lib.rrt_raytracer_destroy(h)

    @property
    def info(self) -> dict:
        """rrt_model_info of the octree this raytracer's GPU set-up built (no host-side tree is built for it)."""
        info = CModelInfo()
        _check(lib().rrt_raytracer_get_octree(self._h, C.byref(info), None, None, None, None, None), "rrt_raytracer_get_octree")
        return {k: getattr(info, k) for k, _ in CModelInfo._fields_}

    @property
    def chain_info(self) -> dict:
        """rrt_raytracer_get_chain_info: chains that have a shortcut record, and the chain nodes those records cover."""
        a = C.c_uint32(0); b = C.c_uint32(0)
        _check(lib().rrt_raytracer_get_chain_info(self._h, C.byref(a), C.byref(b)), "rrt_raytracer_get_chain_info")
        return {"n_chains": a.value, "n_chain_nodes": b.value}

    def octree(self) -> dict:
        """The octree this raytracer's GPU set-up built (rrt_raytracer_get_octree): same dict as SceneData.octree(), plus "info"."""
        info = CModelInfo()
        _check(lib().rrt_raytracer_get_octree(self._h, C.byref(info), None, None, None, None, None), "rrt_raytracer_get_octree")
        n = info.n_nodes
        aabb = np.empty((n, 6)); fc = np.empty(n, np.uint32); tc = np.empty(n, np.uint32); off = np.empty(n + 1, np.uint32)
        idx = np.empty(info.n_tris_in_tree, np.uint32)
        u = lambda a: a.ctypes.data_as(_u32p)
        _check(lib().rrt_raytracer_get_octree(self._h, None, _d(aabb), u(fc), u(tc), u(off), u(idx)), "rrt_raytracer_get_octree")
        return dict(aabb=aabb, first_child=fc, tri_count=tc, own_off=off, own_idx=idx, max_depth=info.max_depth,
                    info={k: getattr(info, k) for k, _ in CModelInfo._fields_})

    def buffer(self, name: str) -> np.ndarray:
        """Raw bytes of one scene buffer in HBM (rrt_raytracer_get_buffer; tests compare the GPU set-up with the host set-up)."""
        which = BUFFERS.index(name)
        nb = C.c_size_t(0)
        _check(lib().rrt_raytracer_get_buffer(self._h, which, None, 0, C.byref(nb)), "rrt_raytracer_get_buffer")
        out = np.empty(nb.value, np.uint8)
        _check(lib().rrt_raytracer_get_buffer(self._h, which, out.ctypes.data_as(_P), nb.value, None), "rrt_raytracer_get_buffer")
        return out

    # the camera (rrt.h: rrt_camera).  Blocking; no frame of this raytracer may be in flight.
    def set_camera(self, eye, right=(1.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), forward=(0.0, 0.0, 1.0)) -> None:
        """rrt_raytracer_set_camera: frames are taken from `eye`; the ray through scene point (a, b, c) has direction right*a + up*b + forward*c.  A new eye
        recomputes the exactness guard on the GPU; an unchanged eye (a pure rotation) costs nothing."""
        c = CCamera(_vec3(eye), _vec3(right), _vec3(up), _vec3(forward))
        _check(lib().rrt_raytracer_set_camera(self._h, C.byref(c)), "rrt_raytracer_set_camera")

    def look_at(self, eye, target, up=(0.0, 1.0, 0.0)) -> None:
        self.set_camera(**look_at(eye, target, up))

    def reset_camera(self) -> None:
        """Back to the creation pose: eye = origin, looking down +z with y up."""
        _check(lib().rrt_raytracer_set_camera(self._h, None), "rrt_raytracer_set_camera")

    def camera(self) -> dict:
        c = CCamera()
        _check(lib().rrt_raytracer_get_camera(self._h, C.byref(c)), "rrt_raytracer_get_camera")
        return _camera_dict(c)

    # scene updates (rrt.h: rrt_raytracer_set_lights, rrt_raytracer_set_triangles).  No launch of this raytracer may be in flight.
    def set_lights(self, lights: Iterable[Light]) -> None:
        """rrt_raytracer_set_lights: the light list of every launch from now on, in this order (host work only)."""
        lights = list(lights)
        cl = (CLight * max(1, len(lights)))()
        for i, l in enumerate(lights):
            cl[i] = CLight(l.kind, 0, float(l.intensity), l.v._c())
        _check(lib().rrt_raytracer_set_lights(self._h, cl, len(lights)), "rrt_raytracer_set_lights")

    def lights(self) -> list:
        """rrt_raytracer_get_lights: the list the kernels get, as Light objects."""
        n = C.c_uint32(0)
        _check(lib().rrt_raytracer_get_lights(self._h, None, 0, C.byref(n)), "rrt_raytracer_get_lights")
        cl = (CLight * max(1, n.value))()
        _check(lib().rrt_raytracer_get_lights(self._h, cl, n.value, C.byref(n)), "rrt_raytracer_get_lights")
        return [Light(l.kind, l.intensity, Vector3d(l.v.x, l.v.y, l.v.z)) for l in cl[:n.value]]

    def set_materials(self, materials: Sequence[dict]) -> None:
        """rrt_raytracer_set_materials (blocking): a new material table (dicts ka, kd, ks, ns, kr, tex, bump) over the resident one, of the same length; textures,
        scene and measured variants stay.  All or nothing."""
        materials = list(materials)
        cm = (CMaterial * max(1, len(materials)))()
        for i, m in enumerate(materials):
            cm[i] = CMaterial(Vec3(*m["ka"]), Vec3(*m["kd"]), Vec3(*m["ks"]), float(m["ns"]), float(m["kr"]), int(m["tex"]), int(m.get("bump", -1)))
        _check(lib().rrt_raytracer_set_materials(self._h, cm, len(materials)), "rrt_raytracer_set_materials")

    def materials(self) -> list:
        """rrt_raytracer_get_materials: the table in force, as the dicts SceneData.materials() returns."""
        n = C.c_uint32(0)
        _check(lib().rrt_raytracer_get_materials(self._h, None, 0, C.byref(n)), "rrt_raytracer_get_materials")
        cm = (CMaterial * max(1, n.value))()
        _check(lib().rrt_raytracer_get_materials(self._h, cm, n.value, C.byref(n)), "rrt_raytracer_get_materials")
        v = lambda a: (a.x, a.y, a.z)
        return [dict(ka=v(m.ka), kd=v(m.kd), ks=v(m.ks), ns=m.ns, kr=m.kr, tex=m.tex, bump=m.bump) for m in cm[:n.value]]

    def set_triangles(self, pos, uv, nrm, mat, root=None) -> None:
        """rrt_raytracer_set_triangles (blocking): new triangles from host arrays ([n,3,3] float64 x 3, [n] uint32 indexing the resident materials); octree,
        index and records are rebuilt on the GPU, everything else stays resident.  root=None: the root box in force.  All or nothing."""
        pos = np.ascontiguousarray(pos, np.float64).reshape(-1, 9); uv = np.ascontiguousarray(uv, np.float64).reshape(-1, 9)
        nrm = np.ascontiguousarray(nrm, np.float64).reshape(-1, 9); mat = np.ascontiguousarray(mat, np.uint32).reshape(-1)
        n = pos.shape[0]
        if not (uv.shape[0] == nrm.shape[0] == mat.shape[0] == n):
            raise ValueError(f"set_triangles: {n} positions, {uv.shape[0]} uv, {nrm.shape[0]} normals, {mat.shape[0]} material indices")
        r = None if root is None else (C.c_double * 6)(*map(float, root))
        _check(lib().rrt_raytracer_set_triangles(self._h, n, _d(pos), _d(uv), _d(nrm), mat.ctypes.data_as(_u32p), r), "rrt_raytracer_set_triangles")

    def set_triangles_from(self, pos_t, uv_t, nrm_t, mat_t, root=None, stream: Optional[int] = None) -> None:
        """rrt_raytracer_set_triangles_device (blocking): the same from torch tensors on this raytracer's device -- pos_t / uv_t / nrm_t float64 of 9 n
        elements, mat_t of n four-byte integers -- read where they lie.  The build waits for the work `stream` (default: the current torch stream) holds, so
        the kernels that write the tensors need not have finished.  ValueError, before any call, for a tensor that is not on a GPU, not contiguous or of the
        wrong dtype or size."""
        import torch
        try:
            assert getattr(pos_t, "is_cuda", False), "pos: not a device tensor"
            n, rem = divmod(pos_t.numel(), 9)
            assert rem == 0, "pos: the element count is not a multiple of 9"
            for t, name in ((pos_t, "pos"), (uv_t, "uv"), (nrm_t, "nrm")):
                _device_tensor(t, 9 * n, 8, name)
                assert t.dtype == torch.float64, f"{name}: want float64, got {t.dtype}"
            _device_tensor(mat_t, n, 4, "mat")
            assert mat_t.dtype in (torch.int32, getattr(torch, "uint32", torch.int32)), f"mat: want a 4-byte integer dtype, got {mat_t.dtype}"
            for t, name in ((pos_t, "pos"), (uv_t, "uv"), (nrm_t, "nrm"), (mat_t, "mat")):
                assert t.device.index in (None, self.device), f"{name}: on device {t.device.index}, the raytracer is on {self.device}"
        except AssertionError as e:
            raise ValueError(f"set_triangles_from: {e}") from None
        r = None if root is None else (C.c_double * 6)(*map(float, root))
        _check(lib().rrt_raytracer_set_triangles_device(self._h, n, _P(pos_t.data_ptr()), _P(uv_t.data_ptr()), _P(nrm_t.data_ptr()), _P(mat_t.data_ptr()), r,
                                                        _P(_stream(stream))), "rrt_raytracer_set_triangles_device")

    def release_update_memory(self) -> None:
        """rrt_raytracer_release_update_memory: frees the device memory kept between set_triangles calls (the next one allocates again)."""
        _check(lib().rrt_raytracer_release_update_memory(self._h), "rrt_raytracer_release_update_memory")

    # raytracer.rs:29, batched
    def get_ray_colours(self, origins, dirs) -> np.ndarray:
        o = np.ascontiguousarray(origins, np.float64).reshape(-1, 3); d = np.ascontiguousarray(dirs, np.float64).reshape(-1, 3)
        assert o.shape == d.shape
        out = np.empty(o.shape[0], np.uint32)
        _check(lib().rrt_get_ray_colours(self._h, o.shape[0], _d(o), _d(d), out.ctypes.data_as(_u32p)), "rrt_get_ray_colours")
        return out

    def get_ray_colour(self, origin: Vector3d, direction: Vector3d) -> int:
        return int(self.get_ray_colours([[origin.x, origin.y, origin.z]], [[direction.x, direction.y, direction.z]])[0])

    # ray.rs:96-168, batched
    def intersect_rays(self, origins, dirs, max_t=None):
        o = np.ascontiguousarray(origins, np.float64).reshape(-1, 3); d = np.ascontiguousarray(dirs, np.float64).reshape(-1, 3)
        n = o.shape[0]
        mt = None if max_t is None else np.ascontiguousarray(np.broadcast_to(np.asarray(max_t, np.float64), (n,)))
        hit = np.empty(n, np.uint8); t = np.empty(n); u = np.empty(n); v = np.empty(n); tri = np.empty(n, np.uint32)
        _check(lib().rrt_intersect_rays(self._h, n, _d(o), _d(d), None if mt is None else _d(mt), hit.ctypes.data_as(_u8p), _d(t), _d(u), _d(v),
                                        tri.ctypes.data_as(_u32p)), "rrt_intersect_rays")
        return hit.astype(bool), t, u, v, tri

    # Some/None of the same walk (rrt.h: rrt_occluded_rays): the reference's shadow query without its negation
    def occluded(self, origins, dirs, max_t=None) -> np.ndarray:
        o = np.ascontiguousarray(origins, np.float64).reshape(-1, 3); d = np.ascontiguousarray(dirs, np.float64).reshape(-1, 3)
        assert o.shape == d.shape
        n = o.shape[0]
        mt = None if max_t is None else np.ascontiguousarray(np.broadcast_to(np.asarray(max_t, np.float64), (n,)))
        out = np.empty(n, np.uint8)
        _check(lib().rrt_occluded_rays(self._h, n, _d(o), _d(d), None if mt is None else _d(mt), out.ctypes.data_as(_u8p)), "rrt_occluded_rays")
        return out.astype(bool)

    # device-resident ray batches (rrt.h: rrt_intersect_rays_device): origins_t / dirs_t are float64 device tensors of 3 n elements, max_t_t of n; enqueued, not synchronised
    def occluded_into(self, origins_t, dirs_t, out_t, max_t_t=None, stream: Optional[int] = None):
        """rrt_occluded_rays_device: out_t = device tensor of n one-byte elements, 1 = occluded."""
        n = _ray_batch(origins_t, dirs_t, max_t_t)
        _device_tensor(out_t, n, 1, "out")
        _check(lib().rrt_occluded_rays_device(self._h, n, _P(origins_t.data_ptr()), _P(dirs_t.data_ptr()), _P(max_t_t.data_ptr()) if max_t_t is not None else None,
                                              _P(out_t.data_ptr()), _P(_stream(stream))), "rrt_occluded_rays_device")

    def intersect_rays_into(self, origins_t, dirs_t, out: dict, max_t_t=None, stream: Optional[int] = None):
        """rrt_intersect_rays_device: out = {name: device tensor of n elements} for any subset of hit (1 byte), t, u, v (float64), tri (4 bytes); the others are not
        computed."""
        n = _ray_batch(origins_t, dirs_t, max_t_t)
        assert set(out) <= set(PLANES[:5]), sorted(out)
        for name, t in out.items():
            _device_tensor(t, n, np.dtype(PLANE_DTYPES[name]).itemsize, name)
        p = [_P(out[name].data_ptr()) if name in out else None for name in PLANES[:5]]
        _check(lib().rrt_intersect_rays_device(self._h, n, _P(origins_t.data_ptr()), _P(dirs_t.data_ptr()), _P(max_t_t.data_ptr()) if max_t_t is not None else None,
                                               *p, _P(_stream(stream))), "rrt_intersect_rays_device")

    def get_ray_colours_into(self, origins_t, dirs_t, colours_t, stream: Optional[int] = None):
        """rrt_get_ray_colours_device: colours_t = device tensor of n four-byte elements, 0x00RRGGBB."""
        n = _ray_batch(origins_t, dirs_t, None)
        _device_tensor(colours_t, n, 4, "colours")
        _check(lib().rrt_get_ray_colours_device(self._h, n, _P(origins_t.data_ptr()), _P(dirs_t.data_ptr()), _P(colours_t.data_ptr()), _P(_stream(stream))),
               "rrt_get_ray_colours_device")

    def tune_rays(self, origins_t, dirs_t, max_t_t=None) -> int:
        """rrt_tune_rays_device (blocking): measures the three traversal variants on this device-resident batch and keeps the fastest for later per-ray calls;
        returns it (an index into VARIANT_NAMES).  The current torch stream is synchronised first: the measurement runs on the default stream."""
        n = _ray_batch(origins_t, dirs_t, max_t_t)
        import torch
        torch.cuda.current_stream().synchronize()
        v = C.c_uint32(0)
        _check(lib().rrt_tune_rays_device(self._h, n, _P(origins_t.data_ptr()), _P(dirs_t.data_ptr()), _P(max_t_t.data_ptr()) if max_t_t is not None else None,
                                          C.byref(v)), "rrt_tune_rays_device")
        return int(v.value)

    # engine.rs:196-253: chunked draw with an update after every chunk (on_update(fb, first_row, n_rows) stands in for canvas.update())
    def render_progressive(self, width: int, height: int, on_update=None, chunk_rows: int = 50) -> np.ndarray:
        fb = np.empty((height, width), np.uint32)
        UPD = C.CFUNCTYPE(None, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32)
        cb = UPD(lambda user, p, w, h, r0, n: on_update(fb, int(r0), int(n))) if on_update is not None else None
        _check(lib().rrt_render_progressive(self._h, width, height, fb.ctypes.data_as(_u32p), chunk_rows, C.cast(cb, _P) if cb is not None else None, None),
               "rrt_render_progressive")
        return fb

    # engine.rs:186 via the C ABI, host framebuffer
    def render(self, width: int, height: int) -> np.ndarray:
        fb = np.empty((height, width), np.uint32)
        _check(lib().rrt_render(self._h, width, height, fb.ctypes.data_as(_u32p)), "rrt_render")
        return fb

    # device-resident variants (torch tensors are plumbing: data_ptr + current stream)
    def render_into(self, fb_tensor, width: int, height: int, stream: Optional[int] = None):
        assert fb_tensor.is_cuda and fb_tensor.is_contiguous() and fb_tensor.numel() == width * height and fb_tensor.element_size() == 4
        _check(lib().rrt_render_device(self._h, width, height, _P(fb_tensor.data_ptr()), _P(_stream(stream))), "rrt_render_device")

    def render_tiles_into(self, tiles_tensor, width: int, height: int, rank: int, world: int, stream: Optional[int] = None):
        need = tiles_per_rank(width, height, world) * 64
        assert tiles_tensor.is_cuda and tiles_tensor.is_contiguous() and tiles_tensor.numel() == need and tiles_tensor.element_size() == 4
        _check(lib().rrt_render_tiles_device(self._h, width, height, rank, world, _P(tiles_tensor.data_ptr()), _P(_stream(stream))), "rrt_render_tiles_device")

    def detile_into(self, gathered_tensor, fb_tensor, width: int, height: int, world: int, stream: Optional[int] = None):
        assert gathered_tensor.numel() == tiles_per_rank(width, height, world) * 64 * world and fb_tensor.numel() == width * height
        _check(lib().rrt_detile_device(self._h, width, height, world, _P(gathered_tensor.data_ptr()), _P(fb_tensor.data_ptr()), _P(_stream(stream))),
               "rrt_detile_device")

    # visibility buffers (rrt.h: rrt_render_visibility): first-hit geometry of the frame's primary rays.  region = (x0, y0, w, h) in canvas pixels, None = the frame
    def visibility(self, width: int, height: int, region=None, planes=PLANES) -> dict:
        """rrt_render_visibility: {plane: array [h][w][4]} of the region (last index: the sub-sample), only the planes asked for.  hit uint8, t / u / v
        float64, tri uint32 (push order, 0xFFFFFFFF = miss), albedo uint32 0x00RRGGBB."""
        h, w = (height, width) if region is None else (int(region[3]), int(region[2]))
        out = {n: np.empty((h, w, 4), PLANE_DTYPES[n]) for n in planes}
        cv = CVisibility(**{n: a.ctypes.data for n, a in out.items()})
        _check(lib().rrt_render_visibility(self._h, width, height, None if region is None else C.byref(CRegion(*map(int, region))), C.byref(cv)), "rrt_render_visibility")
        return out

    def visibility_into(self, tensors: dict, width: int, height: int, region=None, stream: Optional[int] = None):
        """rrt_render_visibility_device: tensors = {plane: contiguous device tensor of 4*w*h elements of the plane's size}; enqueued, not synchronised."""
        n = 4 * (width * height if region is None else int(region[2]) * int(region[3]))
        for name, t in tensors.items():
            assert t.is_cuda and t.is_contiguous() and t.numel() == n and t.element_size() == np.dtype(PLANE_DTYPES[name]).itemsize, name
        cv = CVisibility(**{name: t.data_ptr() for name, t in tensors.items()})
        _check(lib().rrt_render_visibility_device(self._h, width, height, None if region is None else C.byref(CRegion(*map(int, region))), C.byref(cv),
                                                  _P(_stream(stream))), "rrt_render_visibility_device")

    def pick(self, width: int, height: int, px: int, py: int) -> dict:
        """rrt_pick: what sub-sample 0 of canvas pixel (px, py) sees: dict hit (bool), tri, t, u, v, albedo."""
        r = CPickResult()
        _check(lib().rrt_pick(self._h, width, height, px, py, C.byref(r)), "rrt_pick")
        return dict(hit=bool(r.hit), tri=r.tri, t=r.t, u=r.u, v=r.v, albedo=r.albedo)

    # surface buffers (rrt.h: rrt_render_surface): hit point, shading normal, material index and light mask of the frame's primary rays
    def surface(self, width: int, height: int, region=None, planes=SURFACE_PLANES, visibility=()) -> dict:
        """rrt_render_surface: {plane: array} of the region, only the planes asked for.  point / normal float64 [h][w][4][3], material / lights uint32
        [h][w][4] (material 0xFFFFFFFF = miss; lights: bit k = light k reaches the point), and the visibility planes named in `visibility` ([h][w][4], as
        visibility() returns them) from the same launch."""
        h, w = (height, width) if region is None else (int(region[3]), int(region[2]))
        out = {n: np.empty((h, w, 4, 3) if SURFACE_WIDTHS[n] == 3 else (h, w, 4), SURFACE_DTYPES[n]) for n in planes}
        vis = {n: np.empty((h, w, 4), PLANE_DTYPES[n]) for n in visibility}
        cs = CSurface(**{n: a.ctypes.data for n, a in out.items()})
        cv = CVisibility(**{n: a.ctypes.data for n, a in vis.items()})
        _check(lib().rrt_render_surface(self._h, width, height, None if region is None else C.byref(CRegion(*map(int, region))), C.byref(cv) if vis else None,
                                        C.byref(cs)), "rrt_render_surface")
        out.update(vis)
        return out

    def surface_into(self, tensors: dict, width: int, height: int, region=None, stream: Optional[int] = None):
        """rrt_render_surface_device: tensors = {plane: contiguous device tensor}, keys from SURFACE_PLANES (12*w*h float64 for point / normal, 4*w*h four-byte
        elements for material / lights) and from PLANES (4*w*h elements of the plane's size); enqueued, not synchronised."""
        n = 4 * (width * height if region is None else int(region[2]) * int(region[3]))
        for name, t in tensors.items():
            if name in SURFACE_DTYPES:
                _device_tensor(t, n * SURFACE_WIDTHS[name], np.dtype(SURFACE_DTYPES[name]).itemsize, name)
            else:
                _device_tensor(t, n, np.dtype(PLANE_DTYPES[name]).itemsize, name)
        cs = CSurface(**{name: t.data_ptr() for name, t in tensors.items() if name in SURFACE_DTYPES})
        cv = CVisibility(**{name: t.data_ptr() for name, t in tensors.items() if name not in SURFACE_DTYPES})
        _check(lib().rrt_render_surface_device(self._h, width, height, None if region is None else C.byref(CRegion(*map(int, region))), C.byref(cv), C.byref(cs),
                                               _P(_stream(stream))), "rrt_render_surface_device")

    # shading from kept buffers (rrt.h: rrt_shade_surface): the frame of the planes surface() returned, with the lights and materials in force now
    def shade(self, width: int, height: int, planes: dict, region=None) -> np.ndarray:
        """rrt_shade_surface: planes = dict with point, normal ([h][w][4][3] float64), material, albedo ([h][w][4] uint32) and optionally lights, as
        surface(..., visibility=("albedo",)) returns them for this size and region; returns the region's pixels, [h][w] uint32 0x00RRGGBB.  Without `lights`
        the depth-0 shadow rays are walked again.  Other keys are ignored; a missing required plane is passed as NULL (the library refuses it)."""
        h, w = (height, width) if region is None else (int(region[3]), int(region[2]))
        keep = {}
        for name in ("point", "normal", "material", "lights", "albedo"):
            if planes.get(name) is not None:
                dtype = SURFACE_DTYPES.get(name, np.uint32)
                keep[name] = np.ascontiguousarray(planes[name], dtype)
                want = (h, w, 4, 3) if SURFACE_WIDTHS.get(name) == 3 else (h, w, 4)
                if keep[name].shape != want:
                    raise ValueError(f"shade: plane {name} has shape {keep[name].shape}, want {want}")
        cs = CSurface(**{n: a.ctypes.data for n, a in keep.items() if n != "albedo"})
        cv = CVisibility(**({"albedo": keep["albedo"].ctypes.data} if "albedo" in keep else {}))
        fb = np.empty((h, w), np.uint32)
        _check(lib().rrt_shade_surface(self._h, width, height, None if region is None else C.byref(CRegion(*map(int, region))), C.byref(cv), C.byref(cs),
                                       fb.ctypes.data_as(_u32p)), "rrt_shade_surface")
        return fb

    def shade_into(self, fb_tensor, tensors: dict, width: int, height: int, region=None, stream: Optional[int] = None):
        """rrt_shade_surface_device: tensors = {plane: contiguous device tensor} with point, normal, material, albedo and optionally lights, as surface_into
        filled them; fb_tensor = w*h four-byte elements of the region; enqueued, not synchronised."""
        px = width * height if region is None else int(region[2]) * int(region[3])
        _device_tensor(fb_tensor, px, 4, "fb")
        for name in ("point", "normal", "material", "lights", "albedo"):
            if tensors.get(name) is not None:
                _device_tensor(tensors[name], 4 * px * SURFACE_WIDTHS.get(name, 1), 8 if SURFACE_WIDTHS.get(name) == 3 else 4, name)
        ptr = lambda name: tensors[name].data_ptr() if tensors.get(name) is not None else None
        cs = CSurface(point=ptr("point"), normal=ptr("normal"), material=ptr("material"), lights=ptr("lights"))
        cv = CVisibility(albedo=ptr("albedo"))
        _check(lib().rrt_shade_surface_device(self._h, width, height, None if region is None else C.byref(CRegion(*map(int, region))), C.byref(cv), C.byref(cs),
                                              _P(fb_tensor.data_ptr()), _P(_stream(stream))), "rrt_shade_surface_device")

    # ambient occlusion from kept buffers (rrt.h: rrt_ambient_surface): which of the hemisphere rays `dirs` from every first hit are blocked
    def ambient(self, width: int, height: int, planes: dict, dirs, max_t: float = float("inf"), region=None, outputs=AMBIENT_OUTPUTS) -> dict:
        """rrt_ambient_surface: planes = dict with point, normal ([h][w][4][3] float64) and material ([h][w][4] uint32) as surface() returns them for this size
        and region (other keys are ignored; a missing plane is passed as NULL, which the library refuses); dirs = [n][3] directions in the tangent frame of a
        hit (z along the normal), n <= MAX_AMBIENT_SAMPLES; max_t as occluded() takes it.  Returns {"occluded": [h][w][4] uint32, bit k = ray k is blocked,
        "grey": [h][w] uint32 0x00GGGGGG, the share of open rays}, only the outputs asked for."""
        h, w = (height, width) if region is None else (int(region[3]), int(region[2]))
        keep = {}
        for name in ("point", "normal", "material"):
            if planes.get(name) is not None:
                keep[name] = np.ascontiguousarray(planes[name], SURFACE_DTYPES[name])
                want = (h, w, 4, 3) if SURFACE_WIDTHS[name] == 3 else (h, w, 4)
                if keep[name].shape != want:
                    raise ValueError(f"ambient: plane {name} has shape {keep[name].shape}, want {want}")
        d, cs = _ambient_samples(dirs, max_t)
        out = {n: np.empty((h, w, 4) if n == "occluded" else (h, w), np.uint32) for n in outputs}
        _check(lib().rrt_ambient_surface(self._h, width, height, None if region is None else C.byref(CRegion(*map(int, region))),
                                         C.byref(CSurface(**{n: a.ctypes.data for n, a in keep.items()})), C.byref(cs),
                                         C.byref(CAmbient(**{n: a.ctypes.data for n, a in out.items()}))), "rrt_ambient_surface")
        return out

    def ambient_into(self, out_tensors: dict, plane_tensors: dict, dirs, max_t: float, width: int, height: int, region=None, stream: Optional[int] = None):
        """rrt_ambient_surface_device: plane_tensors = {plane: contiguous device tensor} with point, normal and material as surface_into filled them;
        out_tensors = {"occluded": 4*w*h four-byte elements, "grey": w*h four-byte elements} of the region, either or both; dirs (host, [n][3]) and max_t as
        ambient(); enqueued, not synchronised."""
        px = width * height if region is None else int(region[2]) * int(region[3])
        assert set(out_tensors) <= set(AMBIENT_OUTPUTS), sorted(out_tensors)
        for name, t in out_tensors.items():
            _device_tensor(t, 4 * px if name == "occluded" else px, 4, name)
        for name in ("point", "normal", "material"):
            if plane_tensors.get(name) is not None:
                _device_tensor(plane_tensors[name], 4 * px * SURFACE_WIDTHS[name], np.dtype(SURFACE_DTYPES[name]).itemsize, name)
        ptr = lambda name: plane_tensors[name].data_ptr() if plane_tensors.get(name) is not None else None
        d, cs = _ambient_samples(dirs, max_t)
        _check(lib().rrt_ambient_surface_device(self._h, width, height, None if region is None else C.byref(CRegion(*map(int, region))),
                                                C.byref(CSurface(point=ptr("point"), normal=ptr("normal"), material=ptr("material"))), C.byref(cs),
                                                C.byref(CAmbient(**{n: t.data_ptr() for n, t in out_tensors.items()})), _P(_stream(stream))),
               "rrt_ambient_surface_device")

    # pre-bound launchers for per-frame loops (bench.py): all argument conversion is done once, the returned callable is one ctypes call
    def bind_render(self, fb_tensor, width: int, height: int, stream: Optional[int] = None):
        assert fb_tensor.is_cuda and fb_tensor.is_contiguous() and fb_tensor.numel() == width * height and fb_tensor.element_size() == 4
        fn, h, w_, h_, p, st = lib().rrt_render_device, self._h, C.c_uint32(width), C.c_uint32(height), _P(fb_tensor.data_ptr()), _P(_stream(stream))

        def launch():
            rc = fn(h, w_, h_, p, st)
            if rc != OK:
                _check(rc, "rrt_render_device")
        return launch

    def bind_render_tiles(self, tiles_tensor, width: int, height: int, rank: int, world: int, stream: Optional[int] = None):
        assert tiles_tensor.is_cuda and tiles_tensor.is_contiguous() and tiles_tensor.numel() == tiles_per_rank(width, height, world) * 64
        fn, h, st = lib().rrt_render_tiles_device, self._h, _P(_stream(stream))
        args = (C.c_uint32(width), C.c_uint32(height), C.c_uint32(rank), C.c_uint32(world), _P(tiles_tensor.data_ptr()))

        def launch():
            rc = fn(h, *args, st)
            if rc != OK:
                _check(rc, "rrt_render_tiles_device")
        return launch

    def bind_detile(self, gathered_tensor, fb_tensor, width: int, height: int, world: int, stream: Optional[int] = None):
        assert gathered_tensor.numel() == tiles_per_rank(width, height, world) * 64 * world and fb_tensor.numel() == width * height
        fn, h, st = lib().rrt_detile_device, self._h, _P(_stream(stream))
        args = (C.c_uint32(width), C.c_uint32(height), C.c_uint32(world), _P(gathered_tensor.data_ptr()), _P(fb_tensor.data_ptr()))

        def launch():
            rc = fn(h, *args, st)
            if rc != OK:
                _check(rc, "rrt_detile_device")
        return launch

    def setup_times(self) -> dict:
        """Wall ms of the once-per-scene stages: read, parse, texture decode, octree (model) + index, upload (this raytracer)."""
        t = CSetupTimes()
        _check(lib().rrt_get_setup_times(self.scene_data._h if self.scene_data is not None else None, self._h, C.byref(t)), "rrt_get_setup_times")
        return {n: getattr(t, n) for n, _ in CSetupTimes._fields_}

    def render_registered(self, width: int, height: int, fb: Optional[np.ndarray] = None) -> np.ndarray:
        """rrt_render into a page-locked framebuffer (rrt_host_buffer_register): the frame arrives by one asynchronous DMA."""
        if fb is None:
            fb = np.empty((height, width), np.uint32)
        p = _P(fb.ctypes.data)
        _check(lib().rrt_host_buffer_register(p, fb.nbytes), "rrt_host_buffer_register")
        try:
            _check(lib().rrt_render(self._h, width, height, fb.ctypes.data_as(_u32p)), "rrt_render")
        finally:
            _check(lib().rrt_host_buffer_unregister(p), "rrt_host_buffer_unregister")
        return fb

    def last_stats(self) -> dict:
        s = CStats()
        _check(lib().rrt_last_stats(self._h, C.byref(s)), "rrt_last_stats")
        return {n: getattr(s, n) for n, _ in CStats._fields_}


MULTI_LOOPBACK = 1   # RRT_MULTI_LOOPBACK


class MultiGpu:
    """The N GPUs of one node behind one handle (include/rrt.h, rrt_multi): the screen-tile partition, the RCCL gather to rank 0 and the de-tiling
    all happen inside the library.  MultiGpu(raytracers) = one process driving every GPU (rrt_multi_create); MultiGpu.dist(rt, rank, world, unique_id)
    = one process per GPU (rrt_dist_create; rank 0 makes the id with MultiGpu.unique_id() and the caller broadcasts it)."""

    def __init__(self, raytracers: Sequence["RayTracer"], frames_in_flight: int = 1, loopback: bool = False, _handle=None):
        self._keep = list(raytracers)
        if _handle is not None:
            self._h = _handle
            return
        arr = (_P * len(self._keep))(*[rt._h for rt in self._keep])
        out = _P()
        _check(lib().rrt_multi_create(arr, len(self._keep), frames_in_flight, MULTI_LOOPBACK if loopback else 0, C.byref(out)), "rrt_multi_create")
        self._h = out

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        _check(lib().rrt_dist_unique_id(buf), "rrt_dist_unique_id")
        return buf.raw

    @staticmethod
    def dist(rt: "RayTracer", rank: int, world: int, unique_id: Optional[bytes], frames_in_flight: int = 1) -> "MultiGpu":
        out = _P()
        idbuf = C.create_string_buffer(unique_id, 128) if unique_id is not None else None
        _check(lib().rrt_dist_create(rt._h, rank, world, idbuf, frames_in_flight, C.byref(out)), "rrt_dist_create")
        return MultiGpu([rt], _handle=out)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None:
            _lib.rrt_multi_destroy(h)

    def render(self, width: int, height: int) -> np.ndarray:
        """Blocking Scene::draw_scene over all GPUs, host framebuffer (rrt_render_multi)."""
        fb = np.empty((height, width), np.uint32)
        _check(lib().rrt_render_multi(self._h, width, height, fb.ctypes.data_as(_u32p)), "rrt_render_multi")
        return fb

    def bind_enqueue(self, fb_tensor, width: int, height: int):
        """One ctypes call per frame: trace -> gather -> de-tile enqueued on the next slot (fb_tensor on rank 0's GPU, None elsewhere)."""
        fn, h, w_, h_ = lib().rrt_multi_enqueue, self._h, C.c_uint32(width), C.c_uint32(height)
        p = _P(fb_tensor.data_ptr()) if fb_tensor is not None else _P()

        def enqueue():
            rc = fn(h, w_, h_, p)
            if rc != OK:
                _check(rc, "rrt_multi_enqueue")
        return enqueue

    def sync(self) -> None:
        _check(lib().rrt_multi_sync(self._h), "rrt_multi_sync")

    def last_gather_ms(self) -> float:
        v = C.c_double(-1.0)
        _check(lib().rrt_multi_last_gather_ms(self._h, C.byref(v)), "rrt_multi_last_gather_ms")
        return v.value


def _ambient_samples(dirs, max_t):
    """(the [n][3] float64 array, which must outlive the call, and the rrt_ambient_samples that points at it)"""
    d = np.ascontiguousarray(dirs, np.float64).reshape(-1, 3)
    return d, CAmbientSamples(dirs=d.ctypes.data_as(_dp), n=len(d), max_t=float(max_t))


def _device_tensor(t, n: int, itemsize: int, name: str):
    """What every _into form asserts of a tensor before the library sees its pointer (a numpy array fails here, without a GPU)."""
    assert getattr(t, "is_cuda", False), f"{name}: not a device tensor"
    assert t.is_contiguous() and t.element_size() == itemsize and t.numel() == n, f"{name}: want {n} contiguous elements of {itemsize} bytes"


def _ray_batch(origins_t, dirs_t, max_t_t) -> int:
    """Checks a device-resident ray batch (float64 tensors: origins and directions of 3 n elements, max_t of n or None); returns n."""
    assert getattr(origins_t, "is_cuda", False), "origins: not a device tensor"
    n, rem = divmod(origins_t.numel(), 3)
    assert rem == 0, "origins: the element count is not a multiple of 3"
    _device_tensor(origins_t, 3 * n, 8, "origins"); _device_tensor(dirs_t, 3 * n, 8, "dirs")
    if max_t_t is not None:
        _device_tensor(max_t_t, n, 8, "max_t")
    return n


def _stream(stream: Optional[int]) -> int:
    if stream is not None:
        return stream
    import torch
    return torch.cuda.current_stream().cuda_stream


def tiles_per_rank(width: int, height: int, world: int) -> int:
    return int(lib().rrt_tiles_per_rank(width, height, world))


def tile_owner_map(width: int, height: int, world: int) -> np.ndarray:
    """[tiles_y, tiles_x] rank owning each 8x8-pixel tile (tile k -> k % world) -- host mirror of the kernel's partition."""
    tx, ty = (width + 7) // 8, (height + 7) // 8
    return (np.arange(tx * ty, dtype=np.int64) % world).reshape(ty, tx)


def detile_host(gathered: np.ndarray, width: int, height: int, world: int) -> np.ndarray:
    """Host mirror of rrt_detile_device (used by the gloo tests): gathered[world, tiles_per_rank, 64] -> fb[height, width]."""
    tx, ty = (width + 7) // 8, (height + 7) // 8
    tpr = (tx * ty + world - 1) // world
    g = np.asarray(gathered, np.uint32).reshape(world, tpr, 8, 8)
    k = np.arange(tx * ty)
    tiles = g[k % world, k // world].reshape(ty, tx, 8, 8)
    return tiles.transpose(0, 2, 1, 3).reshape(ty * 8, tx * 8)[:height, :width].copy()


class Canvas:                        # src/scene/engine.rs:123-167 minus the minifb window
    def __init__(self, width: int, height: int, on_update=None):
        self.width, self.height = width, height
        self.buffer = np.zeros((height, width), np.uint32)   # engine.rs:135
        self.on_update = on_update                           # stands in for window.update_with_buffer (engine.rs:162-166); None = no display
        self.updates = 0

    def update(self) -> None:                                # engine.rs:160-167
        self.updates += 1
        if self.on_update is not None:
            self.on_update(self.buffer)


class Scene:                         # src/scene/engine.rs:171-256
    def __init__(self, width: int, height: int, on_update=None):
        self.canvas = Canvas(width, height, on_update)

    def draw_scene(self, rt: RayTracer, progressive: bool = False) -> None:
        """Scene::draw_scene (engine.rs:186).  Default: one HIP launch instead of the rayon row loop, one canvas.update() at the end.
        progressive=True keeps the reference's pacing (engine.rs:196-253): 50 scene rows per chunk, canvas.update() after each."""
        if not progressive:
            self.canvas.buffer = rt.render(self.canvas.width, self.canvas.height)
            self.canvas.update()
            return

        def on_chunk(fb, first_row, n_rows):
            self.canvas.buffer = fb
            self.canvas.update()
        self.canvas.buffer = rt.render_progressive(self.canvas.width, self.canvas.height, on_chunk)
