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


FLAG_NO_CULL, FLAG_LANE_FILTER, FLAG_BUNDLE_FILTER, FLAG_RAY_WALK, FLAG_HOST_SETUP, FLAG_NO_CHAIN_SHORTCUT, FLAG_NO_SPECULAR_SKIP, FLAG_NO_COVERAGE, FLAG_COVERAGE_ALWAYS = 1, 2, 4, 8, 16, 32, 64, 128, 256   # RRT_FLAG_*, include/rrt.h
FLAG_NO_WIDE_COVER = 512
# rrt_raytracer_get_coverage_info: state 0 = the last frame ran with a coverage mask, else why not (RRT_COVERAGE_OFF_*, include/rrt.h)
COVERAGE_STATES = ("on", "no_frame", "flag", "no_cull", "suspects", "eye_range", "camera", "pool", "not_whole", "small_frame")
BUFFERS = ("nodes", "geom", "attr", "supers", "cboxes", "child_boxes", "tboxes", "suspects", "oct_box", "oct_first_child", "oct_tri_count", "oct_own_off",
           "oct_own_idx", "slot_tri", "slot_pos", "chains", "tri_slot")   # RRT_BUF_*
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


class CSurface(C.Structure):         # rrt_surface, 32 bytes: host or device pointers, NULL = plane not wanted
    _fields_ = [(n, C.c_void_p) for n in ("point", "normal", "material", "lights")]


class CAmbientSamples(C.Structure):  # rrt_ambient_samples, 24 bytes: dirs = n x 3 host doubles in the tangent frame of a hit
    _fields_ = [("dirs", C.POINTER(C.c_double)), ("n", C.c_uint32), ("_pad", C.c_uint32), ("max_t", C.c_double)]


class CAmbient(C.Structure):         # rrt_ambient, 16 bytes: host or device pointers, NULL = plane not wanted
    _fields_ = [(n, C.c_void_p) for n in ("occluded", "grey")]


class CRaySurface(C.Structure):      # rrt_ray_surface, 96 bytes: host or device pointers, NULL = array not wanted
    _fields_ = [(n, C.c_void_p) for n in ("hit", "t", "u", "v", "tri", "albedo", "point", "normal", "material", "lights", "next_origin", "next_dir")]


class CRayShade(C.Structure):        # rrt_ray_shade, 24 bytes: host or device pointers, NULL = array not wanted
    _fields_ = [(n, C.c_void_p) for n in ("colour", "local", "kr")]


class CRayAmbient(C.Structure):      # rrt_ray_ambient, 16 bytes: host or device pointers, NULL = array not wanted
    _fields_ = [(n, C.c_void_p) for n in ("occluded", "open")]


class CRaySet(C.Structure):          # rrt_ray_set, 128 bytes: host or device pointers, NULL = array not wanted; rec = the twelve arrays of rrt_ray_surface
    _fields_ = [(n, C.c_void_p) for n in ("origins", "dirs", "max_t", "rot")] + [("rec", CRaySurface)]


class CTileTest(C.Structure):        # rrt_tile_test, 72 bytes: a, b host or device pointers
    _fields_ = [(n, C.c_uint32) for n in ("test", "elem_bytes", "per_pixel", "lo", "hi")] + [("set", C.c_uint32 * 8), ("_pad", C.c_uint32), ("a", C.c_void_p), ("b", C.c_void_p)]


MAX_AMBIENT_SAMPLES = 32             # RRT_MAX_AMBIENT_SAMPLES
TILE_TESTS = ("nonzero", "range", "set", "differs")   # RRT_TILE_NONZERO, RRT_TILE_RANGE, RRT_TILE_SET, RRT_TILE_DIFFERS
TILE_KEEP = 0x100                    # RRT_TILE_KEEP, or'ed into rrt_tile_test.test
MAX_TILE_TESTS = 8                   # RRT_MAX_TILE_TESTS
MAX_TILE_LIST = 16777215             # RRT_MAX_TILE_LIST: the longest list render_tile_list_into takes
SELECT_MODES = ("hit", "mirror", "flag")   # RRT_SELECT_HIT, RRT_SELECT_MIRROR, RRT_SELECT_FLAG
DEAD_INDEX = 0xFFFFFFFF              # index of a tail slot of a compacted batch
SORT_KEY_MODES = ("given", "ray", "record")   # RRT_SORT_KEY_GIVEN, RRT_SORT_KEY_RAY, RRT_SORT_KEY_RECORD
DEAD_KEY = 0xFFFFFFFF                # sort key of a dead entry: it sorts last
ORDER_ROWS, ORDER_TILES = 0, 1       # RRT_ORDER_ROWS, RRT_ORDER_TILES: the entry order of a frame's ray batch
FRAME_RAY_ARRAYS = ("origins", "dirs", "max_t")   # what rrt_frame_rays writes, in its order: [n][3], [n][3], [n] float64

# The plane table: every plane of rrt_visibility, rrt_surface and rrt_ambient, in the struct's order, as (dtype, elements per sub-sample, True = one value per
# sub-sample, [h][w][4](...), False = one per pixel, [h][w]).  Everything else the binding knows about a plane is derived from it.
_PLANES_OF = {
    CVisibility: dict(hit=(np.uint8, 1, True), t=(np.float64, 1, True), u=(np.float64, 1, True), v=(np.float64, 1, True), tri=(np.uint32, 1, True),
                      albedo=(np.uint32, 1, True)),
    CSurface: dict(point=(np.float64, 3, True), normal=(np.float64, 3, True), material=(np.uint32, 1, True), lights=(np.uint32, 1, True)),
    CAmbient: dict(occluded=(np.uint32, 1, True), grey=(np.uint32, 1, False)),
}
PLANE_TABLE = {n: row for rows in _PLANES_OF.values() for n, row in rows.items()}
# rrt_ray_surface: the visibility and surface planes' rows per RAY of a batch ([n], [n][3]) and the two vectors of the reference's next ray
_PLANES_OF[CRaySurface] = dict(**_PLANES_OF[CVisibility], **_PLANES_OF[CSurface], next_origin=(np.float64, 3, True), next_dir=(np.float64, 3, True))
PLANES = tuple(_PLANES_OF[CVisibility])                                       # the planes of rrt_visibility, in its order
PLANE_DTYPES = {n: row[0] for n, row in _PLANES_OF[CVisibility].items()}
SURFACE_PLANES = tuple(_PLANES_OF[CSurface])                                  # the planes of rrt_surface, in its order
SURFACE_DTYPES = {n: row[0] for n, row in _PLANES_OF[CSurface].items()}
SURFACE_WIDTHS = {n: row[1] for n, row in _PLANES_OF[CSurface].items()}       # elements per sub-sample
AMBIENT_OUTPUTS = tuple(_PLANES_OF[CAmbient])                                 # the planes of rrt_ambient, in its order: [h][w][4] masks, [h][w] pixels
SHADE_INPUTS = SURFACE_PLANES + ("albedo",)                                   # what rrt_shade_surface reads (lights optional)
AMBIENT_INPUTS = SURFACE_PLANES[:3]                                           # what rrt_ambient_surface reads
RAY_SURFACE_PLANES = tuple(_PLANES_OF[CRaySurface])                           # the arrays of rrt_ray_surface, in its order
# rrt_ray_shade: per RAY the colour, the unquantised local colour and the kr of the hit its record holds
_PLANES_OF[CRayShade] = dict(colour=(np.uint32, 1, True), local=(np.float64, 3, True), kr=(np.float64, 1, True))
RAY_SHADE_OUTPUTS = tuple(_PLANES_OF[CRayShade])                              # the arrays of rrt_ray_shade, in its order
RAY_SHADE_INPUTS = SHADE_INPUTS                                               # what rrt_shade_rays reads of an rrt_ray_surface (lights optional)
# rrt_ray_ambient: per RAY the mask of occluded hemisphere rays and the count of open ones
_PLANES_OF[CRayAmbient] = dict(occluded=(np.uint32, 1, True), open=(np.uint32, 1, True))
RAY_AMBIENT_OUTPUTS = tuple(_PLANES_OF[CRayAmbient])                          # the arrays of rrt_ray_ambient, in its order
RAY_AMBIENT_INPUTS = AMBIENT_INPUTS                                           # what rrt_ambient_rays reads of an rrt_ray_surface
RESOLVE_INPUTS = ("t", "u", "v", "tri")                                       # what rrt_resolve_hits reads of an rrt_ray_surface (u, v: not for point and material alone)
RESOLVE_OUTPUTS = RAY_SURFACE_PLANES[5:]                                      # ... and what it writes there: albedo, point, normal, material, lights, next_origin, next_dir
# rrt_ray_set: per ENTRY of a batch the ray, its bound, the rotation of its ambient fan and the twelve arrays of its record
_PLANES_OF[CRaySet] = dict(origins=(np.float64, 3, True), dirs=(np.float64, 3, True), max_t=(np.float64, 1, True), rot=(np.float64, 2, True), **_PLANES_OF[CRaySurface])
RAY_SET_ARRAYS = tuple(_PLANES_OF[CRaySet])                                   # the arrays of rrt_ray_set, in its order


class CModelInfo(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("n_tris", "n_tris_in_tree", "n_nodes", "max_depth", "n_mats", "n_tex", "root_own_count", "max_own_count")]


class CStats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("width", C.c_uint32), ("height", C.c_uint32), ("rays_primary", C.c_uint64), ("scene_bytes", C.c_uint64),
                ("filter_variant", C.c_uint32), ("origin_plane_triangles", C.c_uint32),
                ("filter_pad", C.c_double), ("filter_alpha_unit", C.c_double), ("filter_delta_unit", C.c_double)]


class CSetupTimes(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("read_ms", "parse_ms", "texture_ms", "octree_ms", "index_ms", "upload_ms", "hip_init_ms", "create_ms", "gpu_setup")]


# every struct of include/rrt.h and the class that mirrors it (tests/test_abi.py compares sizes and offsets with what the header's compiler gives)
STRUCTS = {"rrt_vec3": Vec3, "rrt_light": CLight, "rrt_material": CMaterial, "rrt_texture": CTexture, "rrt_options": COptions, "rrt_camera": CCamera,
           "rrt_region": CRegion, "rrt_visibility": CVisibility, "rrt_pick_result": CPickResult, "rrt_surface": CSurface,
           "rrt_ambient_samples": CAmbientSamples, "rrt_ambient": CAmbient, "rrt_ray_surface": CRaySurface, "rrt_ray_shade": CRayShade, "rrt_ray_ambient": CRayAmbient,
           "rrt_ray_set": CRaySet, "rrt_tile_test": CTileTest,
           "rrt_model_info": CModelInfo, "rrt_stats": CStats, "rrt_setup_times": CSetupTimes}

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
    "rrt_render_region_device": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.POINTER(CRegion), _P, C.c_uint32, _P]),
    "rrt_render_region": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.POINTER(CRegion), _u32p, C.c_uint32]),
    "rrt_render_tile_list_device": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint32, _P, _P, _P, _P]),
    "rrt_render_visibility_tile_list_device": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint32, _P, _P, C.POINTER(CVisibility), _P]),
    "rrt_render_surface_tile_list_device": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint32, _P, _P, C.POINTER(CVisibility), C.POINTER(CSurface), _P]),
    "rrt_shade_surface_tile_list_device": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint32, _P, _P, C.POINTER(CVisibility), C.POINTER(CSurface), _P, _P]),
    "rrt_ambient_surface_tile_list_device": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint32, _P, _P, C.POINTER(CSurface), C.POINTER(CAmbientSamples), C.POINTER(CAmbient), _P]),
    "rrt_mark_tiles_device": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.POINTER(CRegion), C.POINTER(CTileTest), _P, _P]),
    "rrt_mark_tiles": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.POINTER(CRegion), C.POINTER(CTileTest), _u8p]),
    "rrt_select_tiles_device": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.POINTER(CRegion), C.POINTER(CTileTest), C.c_uint32, _P, _P, _P, _P, C.c_size_t, _P]),
    "rrt_select_tiles": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.POINTER(CRegion), C.POINTER(CTileTest), C.c_uint32, _u32p, _u32p]),
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
    "rrt_surface_rays": (C.c_int, [_P, C.c_uint32, _dp, _dp, _dp, C.POINTER(CRaySurface)]),
    "rrt_surface_rays_device": (C.c_int, [_P, C.c_uint32, _P, _P, _P, C.POINTER(CRaySurface), _P]),
    "rrt_shade_rays": (C.c_int, [_P, C.c_uint32, _dp, C.POINTER(CRaySurface), C.c_uint32, C.POINTER(CRayShade)]),
    "rrt_shade_rays_device": (C.c_int, [_P, C.c_uint32, _P, C.POINTER(CRaySurface), C.c_uint32, C.POINTER(CRayShade), _P]),
    "rrt_ambient_rays": (C.c_int, [_P, C.c_uint32, C.POINTER(CRaySurface), _dp, C.POINTER(CAmbientSamples), C.POINTER(CRayAmbient)]),
    "rrt_ambient_rays_device": (C.c_int, [_P, C.c_uint32, C.POINTER(CRaySurface), _P, C.POINTER(CAmbientSamples), C.POINTER(CRayAmbient), _P]),
    "rrt_resolve_hits": (C.c_int, [_P, C.c_uint32, _dp, _dp, C.POINTER(CRaySurface)]),
    "rrt_resolve_hits_device": (C.c_int, [_P, C.c_uint32, _P, _P, C.POINTER(CRaySurface), _P]),
    "rrt_compact_scratch_bytes": (C.c_size_t, [C.c_uint32]),
    "rrt_compact_rays_device": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P, C.POINTER(CRaySet), C.POINTER(CRaySet), _P, _P, _P, C.c_size_t, _P]),
    "rrt_compact_rays": (C.c_int, [_P, C.c_uint32, C.c_uint32, _u8p, C.POINTER(CRaySet), C.POINTER(CRaySet), _u32p, _u32p]),
    "rrt_scatter_rays_device": (C.c_int, [_P, C.c_uint32, _P, C.c_uint32, _P, _P, _P]),
    "rrt_scatter_rays": (C.c_int, [_P, C.c_uint32, _u32p, C.c_uint32, _P, _P]),
    "rrt_sort_scratch_bytes": (C.c_size_t, [C.c_uint32]),
    "rrt_sort_rays_device": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P, C.POINTER(CRaySet), C.POINTER(CRaySet), _P, _P, _P, _P, C.c_size_t, _P]),
    "rrt_sort_rays": (C.c_int, [_P, C.c_uint32, C.c_uint32, _u32p, C.POINTER(CRaySet), C.POINTER(CRaySet), _u32p, _u32p, _u32p]),
    "rrt_frame_ray_count": (C.c_uint32, [C.c_uint32, C.c_uint32, C.POINTER(CRegion), C.c_uint32]),
    "rrt_frame_rays_device": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.POINTER(CRegion), C.c_uint32, _P, _P, _P, _P]),
    "rrt_frame_rays": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.POINTER(CRegion), C.c_uint32, _dp, _dp, _dp]),
    "rrt_mix_rays_device": (C.c_int, [_P, C.c_uint32, _P, _P, _P, _P, _P, _P]),
    "rrt_mix_rays": (C.c_int, [_P, C.c_uint32, _u32p, _dp, _dp, _u32p, _u32p]),
    "rrt_mix_pixels_device": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.POINTER(CRegion), C.c_uint32, _P, _P, _P]),
    "rrt_mix_pixels": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.POINTER(CRegion), C.c_uint32, _u32p, _u32p]),
    "rrt_wavefront_work_bytes": (C.c_size_t, [_P, C.c_uint32, C.c_uint32, C.POINTER(CRegion), C.c_uint32]),
    "rrt_render_wavefront_device": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.POINTER(CRegion), C.c_uint32, _P, _P, C.c_size_t, _P]),
    "rrt_render_wavefront": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.POINTER(CRegion), C.c_uint32, _u32p]),
    # the counted device forms (rrt.h: COUNTED DEVICE FORMS): the device form with the bound, a device pointer, directly after n
    "rrt_intersect_rays_counted_device": (C.c_int, [_P, C.c_uint32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "rrt_get_ray_colours_counted_device": (C.c_int, [_P, C.c_uint32, _P, _P, _P, _P, _P]),
    "rrt_occluded_rays_counted_device": (C.c_int, [_P, C.c_uint32, _P, _P, _P, _P, _P, _P]),
    "rrt_surface_rays_counted_device": (C.c_int, [_P, C.c_uint32, _P, _P, _P, _P, C.POINTER(CRaySurface), _P]),
    "rrt_shade_rays_counted_device": (C.c_int, [_P, C.c_uint32, _P, _P, C.POINTER(CRaySurface), C.c_uint32, C.POINTER(CRayShade), _P]),
    "rrt_ambient_rays_counted_device": (C.c_int, [_P, C.c_uint32, _P, C.POINTER(CRaySurface), _P, C.POINTER(CAmbientSamples), C.POINTER(CRayAmbient), _P]),
    "rrt_resolve_hits_counted_device": (C.c_int, [_P, C.c_uint32, _P, _P, _P, C.POINTER(CRaySurface), _P]),
    "rrt_compact_rays_counted_device": (C.c_int, [_P, C.c_uint32, _P, C.c_uint32, _P, C.POINTER(CRaySet), C.POINTER(CRaySet), _P, _P, _P, C.c_size_t, _P]),
    "rrt_scatter_rays_counted_device": (C.c_int, [_P, C.c_uint32, _P, _P, C.c_uint32, _P, _P, _P]),
    "rrt_mix_rays_counted_device": (C.c_int, [_P, C.c_uint32, _P, _P, _P, _P, _P, _P, _P]),
    "rrt_raytracer_get_octree": (C.c_int, [_P, C.POINTER(CModelInfo), _dp, _u32p, _u32p, _u32p, _u32p]),
    "rrt_raytracer_get_buffer": (C.c_int, [_P, C.c_uint32, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "rrt_raytracer_get_chain_info": (C.c_int, [_P, _u32p, _u32p]),
    "rrt_raytracer_get_coverage_info": (C.c_int, [_P, _u32p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "rrt_raytracer_get_coverage_mask": (C.c_int, [_P, _u32p, C.c_uint64]),
    "rrt_raytracer_get_wide_cover_info": (C.c_int, [_P, _u32p, C.POINTER(C.c_uint64)]),
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


def _call(name: str, *args) -> None:
    """One library call by its entry point's name; a status other than RRT_OK raises RrtError naming it."""
    _check(getattr(lib(), name)(*args), name)


def device_count() -> int:
    n = C.c_int(0)
    _call("rrt_device_count", C.byref(n))
    return n.value


def tiles_per_rank(width: int, height: int, world: int) -> int:
    return int(lib().rrt_tiles_per_rank(width, height, world))


# ---------------------------------------------------------------------------------------------- marshalling: one helper per kind of argument
def _host_pointer(ptype):
    """array -> the pointer of this type the library reads or fills (None = NULL)"""
    return lambda a: None if a is None else a.ctypes.data_as(ptype)


_d, _u32, _u8 = _host_pointer(_dp), _host_pointer(_u32p), _host_pointer(_u8p)


def _ptr(t):
    """A device tensor as the void* the library gets (None = NULL)."""
    return None if t is None else _P(t.data_ptr())


def _stream(stream: Optional[int]) -> int:
    if stream is not None:
        return stream
    import torch
    return torch.cuda.current_stream().cuda_stream


def _vec3(v) -> Vec3:
    """A Vector3d or any three numbers."""
    return v._c() if isinstance(v, Vector3d) else Vec3(*map(float, v))


def _tuple3(v: Vec3) -> tuple:
    return (v.x, v.y, v.z)


def _struct_dict(s: C.Structure) -> dict:
    return {n: getattr(s, n) for n, _ in s._fields_}


def _camera_dict(c: CCamera) -> dict:
    return {n: _tuple3(v) for n, v in _struct_dict(c).items()}


def _root(root):
    """A root box as six doubles (None = NULL: the default box, or the one in force)."""
    return None if root is None else (C.c_double * 6)(*map(float, root))


def _array(ctype, n: int):
    """n elements of `ctype`, zeroed; at least one, so that an empty list still has an address."""
    return (ctype * max(1, n))()


def _c_lights(lights: Iterable["Light"]):
    """(rrt_light array of at least one element, the number of lights)"""
    lights = list(lights)
    cl = _array(CLight, len(lights))
    for i, l in enumerate(lights):
        cl[i] = CLight(l.kind, 0, float(l.intensity), l.v._c())
    return cl, len(lights)


def _c_materials(materials: Sequence[dict]):
    """(rrt_material array of at least one element, the number of materials); dicts ka, kd, ks, ns, kr, tex and optionally bump (absent = -1, none)."""
    materials = list(materials)
    cm = _array(CMaterial, len(materials))
    for i, m in enumerate(materials):
        cm[i] = CMaterial(Vec3(*m["ka"]), Vec3(*m["kd"]), Vec3(*m["ks"]), float(m["ns"]), float(m["kr"]), int(m["tex"]), int(m.get("bump", -1)))
    return cm, len(materials)


def _material_dicts(cm, n: int) -> list:
    return [dict(ka=_tuple3(m.ka), kd=_tuple3(m.kd), ks=_tuple3(m.ks), ns=m.ns, kr=m.kr, tex=m.tex, bump=m.bump) for m in cm[:n]]


def _counted(name: str, handle, ctype):
    """The getters that report a count: ask for it, then fill an array of that many `ctype` (at least one); returns (array, count)."""
    n = C.c_uint32(0)
    _call(name, handle, None, 0, C.byref(n))
    arr = _array(ctype, n.value)
    _call(name, handle, arr, n.value, C.byref(n))
    return arr, n.value


def _options(surface_offset, max_reflection_depth, viewport, no_cull, box_filter, host_setup, chain_shortcut, specular_skip=True, coverage=True, wide_cover=True) -> COptions:
    flags = ((FLAG_NO_CULL if no_cull else 0) | (FLAG_HOST_SETUP if host_setup else 0) | (0 if chain_shortcut else FLAG_NO_CHAIN_SHORTCUT)
             | (0 if specular_skip else FLAG_NO_SPECULAR_SKIP) | (FLAG_COVERAGE_ALWAYS if coverage == "always" else 0 if coverage else FLAG_NO_COVERAGE)
             | (0 if wide_cover else FLAG_NO_WIDE_COVER)
             | {None: 0, "lane": FLAG_LANE_FILTER, "bundle": FLAG_BUNDLE_FILTER, "ray": FLAG_RAY_WALK}[box_filter])
    return COptions(surface_offset, max_reflection_depth, flags, *map(float, viewport))


def _tri_arrays(pos, uv, nrm, mat):
    """Triangles as the library reads them: pos / uv / nrm [n,9] float64, mat [n] uint32, all contiguous (no copy of an array that already is)."""
    return (*(np.ascontiguousarray(a, np.float64).reshape(-1, 9) for a in (pos, uv, nrm)), np.ascontiguousarray(mat, np.uint32).reshape(-1))


def _scene_args(pos, uv, nrm, mat, materials, textures, root):
    """The ten scene arguments rrt_model_from_arrays and rrt_raytracer_create_from_arrays share, and the arrays they point into (to be kept until the call
    returned).  No copies of arrays that are already contiguous float64 / uint32 / uint8."""
    pos, uv, nrm, mat = _tri_arrays(pos, uv, nrm, mat)
    cm, n_mats = _c_materials(materials)
    keep = [np.ascontiguousarray(t, np.uint8) for t in textures]
    ct = _array(CTexture, len(keep))
    for i, t in enumerate(keep):
        ct[i] = CTexture(_u8(t), t.shape[1], t.shape[0])
    return (pos.shape[0], _d(pos), _d(uv), _d(nrm), _u32(mat), n_mats, cm, len(keep), ct, _root(root)), (pos, uv, nrm, mat, keep)


def _octree_arrays(info: dict):
    """(the dict both octree() methods return, its five arrays as the arguments of rrt_model_get_octree / rrt_raytracer_get_octree)"""
    n = info["n_nodes"]
    o = dict(aabb=np.empty((n, 6)), first_child=np.empty(n, np.uint32), tri_count=np.empty(n, np.uint32), own_off=np.empty(n + 1, np.uint32),
             own_idx=np.empty(info["n_tris_in_tree"], np.uint32))
    return dict(o, max_depth=info["max_depth"]), (_d(o["aabb"]), _u32(o["first_child"]), _u32(o["tri_count"]), _u32(o["own_off"]), _u32(o["own_idx"]))


def _host_rays(origins, dirs, max_t=None):
    """Host rays as the library reads them: origins and directions [n,3] float64, max_t None or n doubles (a scalar is broadcast)."""
    o = np.ascontiguousarray(origins, np.float64).reshape(-1, 3); d = np.ascontiguousarray(dirs, np.float64).reshape(-1, 3)
    assert o.shape == d.shape
    mt = None if max_t is None else np.ascontiguousarray(np.broadcast_to(np.asarray(max_t, np.float64), (o.shape[0],)))
    return o, d, mt


def _device_tensor(t, n: int, itemsize: int, name: str):
    """What every _into form asserts of a tensor before the library sees its pointer (a numpy array fails here, without a GPU)."""
    assert getattr(t, "is_cuda", False), f"{name}: not a device tensor"
    assert t.is_contiguous() and t.element_size() == itemsize and t.numel() == n, f"{name}: want {n} contiguous elements of {itemsize} bytes"


def _bounded(symbol: str, bound_t, handle, n: int) -> tuple:
    """The head of a device-form call -- symbol, handle, n -- and with a bound (rrt.h: COUNTED DEVICE FORMS; a device tensor of one 4-byte element) the counted symbol
    and the bound's pointer behind n.  Without one the call is the uncounted one, untouched."""
    if bound_t is None:
        return symbol, handle, n
    _device_tensor(bound_t, 1, 4, "bound")
    assert symbol.endswith("_device"), symbol
    return symbol[:-len("_device")] + "_counted_device", handle, n, _ptr(bound_t)


def _batch_size(t, per: int, name: str) -> int:
    """n of a device tensor that leads a batch with `per` elements for each of n items"""
    assert getattr(t, "is_cuda", False), f"{name}: not a device tensor"
    n, rem = divmod(t.numel(), per)
    assert rem == 0, f"{name}: the element count is not a multiple of {per}"
    return n


def _tile_list(tiles_t, bound_t) -> tuple:
    """The size checks render_tile_list_into makes of a device-resident tile list and its bound, for the tile-list stages: (n, bound pointer, list pointer)."""
    n = _batch_size(tiles_t, 1, "tiles")
    _device_tensor(tiles_t, n, 4, "tiles")
    if bound_t is not None:
        _device_tensor(bound_t, 1, 4, "bound")
    return n, _ptr(bound_t), _ptr(tiles_t)


def _ray_batch(origins_t, dirs_t, max_t_t) -> int:
    """Checks a device-resident ray batch (float64 tensors: origins and directions of 3 n elements, max_t of n or None); returns n."""
    n = _batch_size(origins_t, 3, "origins")
    _device_tensor(origins_t, 3 * n, 8, "origins"); _device_tensor(dirs_t, 3 * n, 8, "dirs")
    if max_t_t is not None:
        _device_tensor(max_t_t, n, 8, "max_t")
    return n


def _ambient_samples(dirs, max_t):
    """(the [n][3] float64 array, which must outlive the call, and the rrt_ambient_samples that points at it)"""
    d = np.ascontiguousarray(dirs, np.float64).reshape(-1, 3)
    return d, CAmbientSamples(dirs=_d(d), n=len(d), max_t=float(max_t))


def _region(width: int, height: int, region):
    """region = (x0, y0, w, h) in canvas pixels, None = the frame: (rrt_region by reference or NULL, width, height of what the call covers)."""
    if region is None:
        return None, width, height
    x0, y0, w, h = map(int, region)
    return C.byref(CRegion(x0, y0, w, h)), w, h


def _plane_shape(name: str, w: int, h: int) -> tuple:
    _, width, per_sample = PLANE_TABLE[name]
    return (h, w) + ((4,) if per_sample else ()) + ((width,) if width > 1 else ())


def _alloc_planes(cls, names, w: int, h: int) -> dict:
    """{plane: uninitialised host array of the table's shape and dtype for a w x h region}, for planes of the struct `cls`"""
    return {n: np.empty(_plane_shape(n, w, h), _PLANES_OF[cls][n][0]) for n in names}


def _host_planes(what: str, planes: dict, names, w: int, h: int) -> dict:
    """The caller's host planes among `names` as contiguous arrays of the table's dtype; absent or None planes are left out (NULL for the library), a
    wrong shape is a ValueError."""
    keep = {}
    for name in names:
        if planes.get(name) is not None:
            keep[name] = np.ascontiguousarray(planes[name], PLANE_TABLE[name][0])
            if keep[name].shape != _plane_shape(name, w, h):
                raise ValueError(f"{what}: plane {name} has shape {keep[name].shape}, want {_plane_shape(name, w, h)}")
    return keep


def _device_planes(tensors: dict, names, w: int, h: int) -> dict:
    """The caller's device planes among `names`, each checked by _device_tensor against the table; absent or None planes are left out."""
    keep = {}
    for name in names:
        if tensors.get(name) is not None:
            _device_tensor(tensors[name], int(np.prod(_plane_shape(name, w, h))), np.dtype(PLANE_TABLE[name][0]).itemsize, name)
            keep[name] = tensors[name]
    return keep


def _plane_struct(cls, planes: dict):
    """The planes that belong to rrt_visibility / rrt_surface / rrt_ambient `cls`, host arrays or device tensors, by reference; the others stay NULL."""
    return C.byref(cls(**{n: (a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()) for n, a in planes.items() if n in _PLANES_OF[cls]}))


def _ray_plane(name: str, cls=CRaySurface, what: str = "surface_rays"):
    """(dtype, elements per ray) of an array of rrt_ray_surface, or of rrt_ray_shade / rrt_ray_ambient `cls`; an unknown name is a ValueError"""
    if name not in _PLANES_OF[cls]:
        raise ValueError(f"{what}: unknown {'plane' if cls is CRaySurface else 'output'} {name!r}, want names from {tuple(_PLANES_OF[cls])}")
    return _PLANES_OF[cls][name][:2]


def _ray_records(what: str, planes: dict, inputs=RAY_SHADE_INPUTS) -> dict:
    """The arrays of an rrt_ray_surface that a call reads -- `inputs`: rrt_shade_rays' by default -- of the caller's `planes` (host arrays or device tensors):
    {name: (array, dtype, elements per ray)}.  Every name must be one of RAY_SURFACE_PLANES (ValueError otherwise); None and the arrays the call ignores are left
    out (NULL for the library)."""
    rows = {name: (a,) + _ray_plane(name, what=what) for name, a in planes.items()}
    return {name: row for name, row in rows.items() if row[0] is not None and name in inputs}


def _resolve_output(name: str, what: str):
    """(dtype, elements per ray) of an array rrt_resolve_hits writes; any other name is a ValueError"""
    if name not in RESOLVE_OUTPUTS:
        raise ValueError(f"{what}: unknown output {name!r}, want names from {RESOLVE_OUTPUTS}")
    return _ray_plane(name, what=what)


def _ray_set(arrays: dict):
    """An rrt_ray_set of host arrays or device tensors {name: array} with names from RAY_SET_ARRAYS, by reference; None when there are none (NULL)."""
    if not arrays:
        return None
    at = {n: (a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()) for n, a in arrays.items()}
    return C.byref(CRaySet(rec=CRaySurface(**{n: p for n, p in at.items() if n in _PLANES_OF[CRaySurface]}),
                           **{n: p for n, p in at.items() if n not in _PLANES_OF[CRaySurface]}))


def _select(select: str, what: str) -> int:
    if select not in SELECT_MODES:
        raise ValueError(f"{what}: unknown select {select!r}, want one of {SELECT_MODES}")
    return SELECT_MODES.index(select)


def compact_scratch_bytes(n: int) -> int:
    """rrt_compact_scratch_bytes: the device scratch compact_rays_into needs for a batch of n entries."""
    return int(lib().rrt_compact_scratch_bytes(int(n)))


def tile_count(width: int, height: int) -> tuple:
    """(tiles_x, tiles_y) of a frame: the 8x8-pixel tiles rrt_render_tile_list_device numbers ty * tiles_x + tx"""
    return (int(width) + 7) // 8, (int(height) + 7) // 8


def tile_test(kind: str, a, b=None, lo: int = 0, hi: int = 0, values=(), keep: bool = False) -> CTileTest:
    """An rrt_tile_test over the plane `a` (and `b`, for "differs"): numpy arrays for the host forms, device tensors for the _into forms, [h][w] (a framebuffer)
    or [h][w][4] (a sub-sample plane) for the region the call names; elem_bytes is the dtype's item size (1, 4 or 8) and elements are compared as unsigned
    integers.  kind: "nonzero" (x != 0), "range" (lo <= x < hi), "set" (x in `values`, each below 256) or "differs" (a != b).  keep: RRT_TILE_KEEP, the marks
    already there are joined.  The struct keeps its planes alive."""
    if kind not in TILE_TESTS:
        raise ValueError(f"tile_test: unknown kind {kind!r}, want one of {TILE_TESTS}")
    planes = [a] + ([b] if kind == "differs" else [])
    if any(p is None for p in planes):
        raise ValueError(f"tile_test: {kind!r} needs plane {'a' if a is None else 'b'}")
    device = not isinstance(a, np.ndarray)
    if not device:
        planes = [np.ascontiguousarray(p) for p in planes]
    shape = tuple(planes[0].shape)
    if not (len(shape) == 2 or (len(shape) == 3 and shape[2] == 4)):
        raise ValueError(f"tile_test: a plane of shape {shape}, want [h][w] or [h][w][4]")
    size = planes[0].element_size() if device else planes[0].dtype.itemsize
    for p in planes:
        if device:
            assert getattr(p, "is_cuda", False) and p.is_contiguous(), "tile_test: a plane is neither a numpy array nor a contiguous device tensor"
        if tuple(p.shape) != shape or (p.element_size() if device else p.dtype.itemsize) != size:
            raise ValueError("tile_test: planes a and b differ in shape or element size")
    if size not in (1, 4, 8) or (kind in ("range", "set") and size != 4):
        raise ValueError(f"tile_test: {kind!r} over elements of {size} bytes, want {'4' if kind in ('range', 'set') else '1, 4 or 8'}")
    t = CTileTest(test=TILE_TESTS.index(kind) | (TILE_KEEP if keep else 0), elem_bytes=size, per_pixel=4 if len(shape) == 3 else 1, lo=int(lo), hi=int(hi))
    for v in values:
        if not 0 <= int(v) < 256:
            raise ValueError(f"tile_test: value {v} of a set, want 0 to 255")
        t.set[int(v) >> 5] |= 1 << (int(v) & 31)
    at = [p.data_ptr() if device else p.ctypes.data for p in planes]
    t.a, t.b = at[0], (at[1] if len(at) == 2 else None)
    t._planes, t._shape, t._device = planes, shape[:2], device
    return t


def _tile_tests(what: str, tests, w: int, h: int, device: bool):
    """(rrt_tile_test array, count) of tile_test structs for a w x h region, all host (device False) or all device planes; the array keeps the structs alive."""
    tests = [tests] if isinstance(tests, CTileTest) else list(tests)
    if not 1 <= len(tests) <= MAX_TILE_TESTS:
        raise ValueError(f"{what}: {len(tests)} tests, want 1 to {MAX_TILE_TESTS}")
    for t in tests:
        assert getattr(t, "_device", None) is device, f"{what}: a test's planes are {'host arrays' if device else 'device tensors'} (or the struct is not from tile_test)"
        if t._shape != (h, w):
            raise ValueError(f"{what}: a plane of {t._shape[0]} x {t._shape[1]} pixels for a region of {h} x {w}")
    arr = (CTileTest * len(tests))(*tests)
    arr._tests = tests
    return arr, len(tests)


def _key_mode(key: str, what: str) -> int:
    if key not in SORT_KEY_MODES:
        raise ValueError(f"{what}: unknown key {key!r}, want one of {SORT_KEY_MODES}")
    return SORT_KEY_MODES.index(key)


_SORT_KEY_READS = ((), ("origins", "dirs"), ("point", "normal", "material"))   # the arrays of src a key mode needs, per mode of SORT_KEY_MODES


def sort_scratch_bytes(n: int) -> int:
    """rrt_sort_scratch_bytes: the device scratch sort_rays_into needs for a batch of n entries."""
    return int(lib().rrt_sort_scratch_bytes(int(n)))


def _order(order: int, what: str) -> int:
    if order not in (ORDER_ROWS, ORDER_TILES):
        raise ValueError(f"{what}: unknown order {order!r}, want ORDER_ROWS ({ORDER_ROWS}) or ORDER_TILES ({ORDER_TILES})")
    return int(order)


def frame_ray_count(width: int, height: int, region=None, order: int = ORDER_ROWS) -> int:
    """rrt_frame_ray_count: the entries of the ray batch of a region of a frame in `order` -- 4 per pixel in rows order, 64 per 4x4 tile of the frame the region
    touches in tiles order; 0 for arguments the library refuses."""
    return int(lib().rrt_frame_ray_count(int(width), int(height), _region(width, height, region)[0], _order(order, "frame_ray_count")))


def _frame_ray_array(name: str, what: str):
    """(dtype, elements per entry) of an array of rrt_frame_rays; an unknown name is a ValueError"""
    if name not in FRAME_RAY_ARRAYS:
        raise ValueError(f"{what}: unknown array {name!r}, want names from {FRAME_RAY_ARRAYS}")
    return _PLANES_OF[CRaySet][name][:2]


def _bound(name: str, *args):
    """A launcher for per-frame loops: `args` were converted once, the callable is one library call and one comparison (bench.py)."""
    fn = getattr(lib(), name)

    def launch():
        rc = fn(*args)
        if rc != OK:
            _check(rc, name)
    return launch


class _Handle:
    """An object of the library behind self._h, destroyed once with the entry point named by _destroy (never after the library is gone)."""
    _h = None
    _destroy = ""

    def __del__(self):
        h, self._h = self._h, None
        if h and _lib is not None:
            getattr(_lib, self._destroy)(h)


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
SURFACE_OFFSET, MAX_REFLECTION_DEPTH, VIEWPORT = 0.0001, 5, (1.0, 1.0, 1.0)   # rrt_options' defaults: raytracer.rs:17, raytracer.rs:20, engine.rs:113-119


def look_at(eye, target, up=(0.0, 1.0, 0.0)) -> dict:
    """rrt_camera_look_at (host only): the pose at `eye` looking at `target`, left-handed like the reference (x right, y up, z forward), as a dict
    eye / right / up / forward of 3-tuples -- RayTracer.set_camera(**look_at(...)) applies it."""
    c = CCamera()
    _call("rrt_camera_look_at", _vec3(eye), _vec3(target), _vec3(up), C.byref(c))
    return _camera_dict(c)


class SceneData(_Handle):
    """SceneData (scenedata.rs:5-13): triangles in push order + materials + decoded textures + the octree."""
    _destroy = "rrt_model_destroy"

    def __init__(self, handle: int):
        self._h = _P(handle)
        self._info = None

    @property
    def info(self) -> dict:
        """rrt_model_get_info.  Builds the HOST copy of the octree on first use (the default GPU set-up of a RayTracer never needs it), so this is
        also where a too-deep tree (RRT_ERR_DEPTH) is reported on the host side."""
        if self._info is None:
            info = CModelInfo()
            _call("rrt_model_get_info", self._h, C.byref(info))
            self._info = _struct_dict(info)
        return self._info

    @staticmethod
    def from_arrays(pos, uv, nrm, mat, materials: Sequence[dict], textures: Sequence[np.ndarray], root=DEFAULT_ROOT) -> "SceneData":
        """pos/uv/nrm: [n,3,3] float64; mat: [n] uint32; materials: dicts ka,kd,ks,ns,kr,tex,bump; textures: [h,w,3] uint8."""
        scene, _keep = _scene_args(pos, uv, nrm, mat, materials, textures, root)
        out = _P()
        _call("rrt_model_from_arrays", *scene, C.byref(out))
        return SceneData(out.value)

    # --- accessors
    def triangles(self):
        n = self.info["n_tris"]
        pos, uv, nrm, mat = (np.empty((n, 3, 3)), np.empty((n, 3, 3)), np.empty((n, 3, 3)), np.empty(n, np.uint32))
        _call("rrt_model_get_triangles", self._h, _d(pos), _d(uv), _d(nrm), _u32(mat))
        return pos, uv, nrm, mat

    def materials(self) -> list:
        n = self.info["n_mats"]
        cm = _array(CMaterial, n)
        _call("rrt_model_get_materials", self._h, cm)
        return _material_dicts(cm, n)

    def texture(self, i: int) -> np.ndarray:
        t = CTexture()
        _call("rrt_model_get_texture", self._h, i, C.byref(t))
        return np.ctypeslib.as_array(t.rgb, shape=(t.height, t.width, 3)).copy()

    def textures(self) -> list:
        return [self.texture(i) for i in range(self.info["n_tex"])]

    def octree(self) -> dict:
        out, arrays = _octree_arrays(self.info)
        _call("rrt_model_get_octree", self._h, *arrays)
        return out


def parse_obj_file(path: str, root=DEFAULT_ROOT) -> SceneData:
    """fs::read_to_string + parse_obj_file_lines (src/main.rs:28-30, src/file_management/utils.rs:139-213)."""
    out = _P()
    _check(lib().rrt_model_load_obj(os.fsencode(path), _root(root), C.byref(out)), f"parse_obj_file({path})")
    return SceneData(out.value)


def decode_image_file(path: str) -> np.ndarray:
    """The build-owned stand-in for `image::ImageReader::open(..).decode()` (utils.rs:345-350): [h,w,3] uint8."""
    p = _u8p(); w = C.c_uint32(); h = C.c_uint32()
    _check(lib().rrt_decode_image_file(os.fsencode(path), C.byref(p), C.byref(w), C.byref(h)), f"decode_image_file({path})")
    try:
        return np.ctypeslib.as_array(p, shape=(h.value, w.value, 3)).copy()
    finally:
        lib().rrt_free(p)


class RayTracer(_Handle):
    """RayTracer{scene_data, lights, origin} (raytracer.rs:22-26), uploaded once to one MI355X."""
    _destroy = "rrt_raytracer_destroy"

    def __init__(self, scene_data: SceneData, lights: Iterable[Light], origin: Vector3d = DEFAULT_ORIGIN, device: int = 0,
                 surface_offset: float = SURFACE_OFFSET, max_reflection_depth: int = MAX_REFLECTION_DEPTH, viewport=VIEWPORT, no_cull: bool = False,
                 box_filter: Optional[str] = None, host_setup: bool = False, chain_shortcut: bool = True, specular_skip: bool = True, coverage: bool = True, wide_cover: bool = True):
        """no_cull=True (RRT_FLAG_NO_CULL): walk every own list in full, in list order, as ray.rs:119-129; default uses the cluster boxes.
        box_filter: None = rule of thumb on the first frame of a size, measured on the second, "lane" / "bundle" / "ray" = forced (RRT_FLAG_LANE_FILTER / RRT_FLAG_BUNDLE_FILTER /
        RRT_FLAG_RAY_WALK); same pixels.  host_setup=True (RRT_FLAG_HOST_SETUP): octree, index and records built on the host and uploaded (default: built on
        the GPU, csrc/scene_build.hip); same bytes in HBM.  chain_shortcut=False (RRT_FLAG_NO_CHAIN_SHORTCUT): the bundle-filter walk enters every node of a
        one-child chain; same results.  specular_skip=False (RRT_FLAG_NO_SPECULAR_SKIP): every specular term is evaluated, also those the lighting sum absorbs
        bit for bit; same results.  coverage=False (RRT_FLAG_NO_COVERAGE): whole frames run without the coverage pass, every wave walks; coverage="always"
        (RRT_FLAG_COVERAGE_ALWAYS): also frames for which the pass is judged not to pay run with it; same results.  wide_cover=False (RRT_FLAG_NO_WIDE_COVER):
        the pass lists no wide boxes, every covered wave walks its primary rays; same results."""
        self.scene_data, self.origin, self.device = scene_data, origin, device
        cl, n_lights = _c_lights(lights)                       # (not kept: lights() asks the library for the list in force)
        opt = _options(surface_offset, max_reflection_depth, viewport, no_cull, box_filter, host_setup, chain_shortcut, specular_skip, coverage, wide_cover)
        out = _P()
        _call("rrt_raytracer_create", scene_data._h, cl, n_lights, origin._c(), C.byref(opt), device, C.byref(out))
        self._h = out

    @classmethod
    def from_arrays(cls, pos, uv, nrm, mat, materials: Sequence[dict], textures: Sequence[np.ndarray], lights: Iterable[Light], origin: Vector3d = DEFAULT_ORIGIN,
                    device: int = 0, root=DEFAULT_ROOT, no_cull: bool = False, box_filter: Optional[str] = None, specular_skip: bool = True, coverage: bool = True,
                    wide_cover: bool = True) -> "RayTracer":
        """rrt_raytracer_create_from_arrays: the raytracer straight from the host's arrays (no SceneData / rrt_model, no host copy of the scene)."""
        self = cls.__new__(cls)
        self.scene_data, self.origin, self.device = None, origin, device
        scene, _keep = _scene_args(pos, uv, nrm, mat, materials, textures, root)
        cl, n_lights = _c_lights(lights)
        opt = _options(SURFACE_OFFSET, MAX_REFLECTION_DEPTH, VIEWPORT, no_cull, box_filter, False, True, specular_skip, coverage, wide_cover)
        out = _P()
        _call("rrt_raytracer_create_from_arrays", *scene, cl, n_lights, origin._c(), C.byref(opt), device, C.byref(out))
        self._h = out
        return self

    @property
    def info(self) -> dict:
        """rrt_model_info of the octree this raytracer's GPU set-up built (no host-side tree is built for it)."""
        info = CModelInfo()
        _call("rrt_raytracer_get_octree", self._h, C.byref(info), None, None, None, None, None)
        return _struct_dict(info)

    @property
    def chain_info(self) -> dict:
        """rrt_raytracer_get_chain_info: chains that have a shortcut record, and the chain nodes those records cover."""
        a = C.c_uint32(0); b = C.c_uint32(0)
        _call("rrt_raytracer_get_chain_info", self._h, C.byref(a), C.byref(b))
        return {"n_chains": a.value, "n_chain_nodes": b.value}

    def coverage_info(self, count: bool = False) -> dict:
        """rrt_raytracer_get_coverage_info: whether the last frame launch ran with a coverage mask ("state": one of COVERAGE_STATES) and the waves of that frame;
        count=True also waits for the frame, reads its mask back and reports how many waves it proved empty."""
        state = C.c_uint32(0); waves = C.c_uint64(0); empty = C.c_uint64(0)
        _call("rrt_raytracer_get_coverage_info", self._h, C.byref(state), C.byref(waves), C.byref(empty) if count else None)
        out = {"state": COVERAGE_STATES[state.value], "n_waves": waves.value}
        return dict(out, n_proved_empty=empty.value) if count else out

    def wide_cover_info(self) -> dict:
        """rrt_raytracer_get_wide_cover_info: the wide boxes the coverage pass of the last frame launch listed and the waves only they reach (their primary rays were
        tested against those triangles, not walked).  Waits for the frame and reads the counts back; both 0 where that frame ran without a mask."""
        n = C.c_uint32(0); waves = C.c_uint64(0)
        _call("rrt_raytracer_get_wide_cover_info", self._h, C.byref(n), C.byref(waves))
        return {"n_wide": n.value, "n_simple_waves": waves.value}

    def coverage_mask(self) -> Optional[np.ndarray]:
        """rrt_raytracer_get_coverage_mask: the coverage mask of the last frame launch as a bool array [2 tiles_y, 2 tiles_x] indexed [by, bx] -- True where the
        4x4-pixel wave (bx, by) walked, False where the mask proved it empty -- or None where that frame ran without a mask (coverage_info()["state"] != "on").
        Waits for the frame and reads its mask back."""
        if self.coverage_info()["state"] != "on":
            return None
        stats = self.last_stats()
        tiles_x, tiles_y = (stats["width"] + 7) // 8, (stats["height"] + 7) // 8
        words = np.zeros((tiles_x * tiles_y + 7) // 8, np.uint32)
        _call("rrt_raytracer_get_coverage_mask", self._h, _u32(words), words.size)
        by, bx = np.mgrid[0:2 * tiles_y, 0:2 * tiles_x]
        bit = (((by >> 1) * tiles_x + (bx >> 1)) << 2) | ((by & 1) << 1) | (bx & 1)      # coverage_wave_index (csrc/coverage_rule.hpp)
        return ((words[bit >> 5] >> (bit & 31).astype(np.uint32)) & 1).astype(bool)

    def octree(self) -> dict:
        """The octree this raytracer's GPU set-up built (rrt_raytracer_get_octree): same dict as SceneData.octree(), plus "info"."""
        info = self.info
        out, arrays = _octree_arrays(info)
        _call("rrt_raytracer_get_octree", self._h, None, *arrays)
        return dict(out, info=info)

    def buffer(self, name: str) -> np.ndarray:
        """Raw bytes of one scene buffer in HBM (rrt_raytracer_get_buffer; tests compare the GPU set-up with the host set-up)."""
        which = BUFFERS.index(name)
        nb = C.c_size_t(0)
        _call("rrt_raytracer_get_buffer", self._h, which, None, 0, C.byref(nb))
        out = np.empty(nb.value, np.uint8)
        _call("rrt_raytracer_get_buffer", self._h, which, out.ctypes.data_as(_P), nb.value, None)
        return out

    # the camera (rrt.h: rrt_camera).  Blocking; no frame of this raytracer may be in flight.
    def set_camera(self, eye, right=(1.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), forward=(0.0, 0.0, 1.0)) -> None:
        """rrt_raytracer_set_camera: frames are taken from `eye`; the ray through scene point (a, b, c) has direction right*a + up*b + forward*c.  A new eye
        recomputes the exactness guard on the GPU; an unchanged eye (a pure rotation) costs nothing."""
        _call("rrt_raytracer_set_camera", self._h, C.byref(CCamera(_vec3(eye), _vec3(right), _vec3(up), _vec3(forward))))

    def look_at(self, eye, target, up=(0.0, 1.0, 0.0)) -> None:
        self.set_camera(**look_at(eye, target, up))

    def reset_camera(self) -> None:
        """Back to the creation pose: eye = origin, looking down +z with y up."""
        _call("rrt_raytracer_set_camera", self._h, None)

    def camera(self) -> dict:
        c = CCamera()
        _call("rrt_raytracer_get_camera", self._h, C.byref(c))
        return _camera_dict(c)

    # scene updates (rrt.h: rrt_raytracer_set_lights, rrt_raytracer_set_triangles).  No launch of this raytracer may be in flight.
    def set_lights(self, lights: Iterable[Light]) -> None:
        """rrt_raytracer_set_lights: the light list of every launch from now on, in this order (host work only)."""
        _call("rrt_raytracer_set_lights", self._h, *_c_lights(lights))

    def lights(self) -> list:
        """rrt_raytracer_get_lights: the list the kernels get, as Light objects."""
        cl, n = _counted("rrt_raytracer_get_lights", self._h, CLight)
        return [Light(l.kind, l.intensity, Vector3d(*_tuple3(l.v))) for l in cl[:n]]

    def set_materials(self, materials: Sequence[dict]) -> None:
        """rrt_raytracer_set_materials (blocking): a new material table (dicts ka, kd, ks, ns, kr, tex, bump) over the resident one, of the same length; textures,
        scene and measured variants stay.  All or nothing."""
        _call("rrt_raytracer_set_materials", self._h, *_c_materials(materials))

    def materials(self) -> list:
        """rrt_raytracer_get_materials: the table in force, as the dicts SceneData.materials() returns."""
        return _material_dicts(*_counted("rrt_raytracer_get_materials", self._h, CMaterial))

    def set_triangles(self, pos, uv, nrm, mat, root=None) -> None:
        """rrt_raytracer_set_triangles (blocking): new triangles from host arrays ([n,3,3] float64 x 3, [n] uint32 indexing the resident materials); octree,
        index and records are rebuilt on the GPU, everything else stays resident.  root=None: the root box in force.  All or nothing."""
        pos, uv, nrm, mat = _tri_arrays(pos, uv, nrm, mat)
        n = pos.shape[0]
        if not (uv.shape[0] == nrm.shape[0] == mat.shape[0] == n):
            raise ValueError(f"set_triangles: {n} positions, {uv.shape[0]} uv, {nrm.shape[0]} normals, {mat.shape[0]} material indices")
        _call("rrt_raytracer_set_triangles", self._h, n, _d(pos), _d(uv), _d(nrm), _u32(mat), _root(root))

    def set_triangles_from(self, pos_t, uv_t, nrm_t, mat_t, root=None, stream: Optional[int] = None) -> None:
        """rrt_raytracer_set_triangles_device (blocking): the same from torch tensors on this raytracer's device -- pos_t / uv_t / nrm_t float64 of 9 n
        elements, mat_t of n four-byte integers -- read where they lie.  The build waits for the work `stream` (default: the current torch stream) holds, so
        the kernels that write the tensors need not have finished.  ValueError, before any call, for a tensor that is not on a GPU, not contiguous or of the
        wrong dtype or size."""
        import torch
        try:
            n = _batch_size(pos_t, 9, "pos")
            for t, name in ((pos_t, "pos"), (uv_t, "uv"), (nrm_t, "nrm")):
                _device_tensor(t, 9 * n, 8, name)
                assert t.dtype == torch.float64, f"{name}: want float64, got {t.dtype}"
            _device_tensor(mat_t, n, 4, "mat")
            assert mat_t.dtype in (torch.int32, getattr(torch, "uint32", torch.int32)), f"mat: want a 4-byte integer dtype, got {mat_t.dtype}"
            for t, name in ((pos_t, "pos"), (uv_t, "uv"), (nrm_t, "nrm"), (mat_t, "mat")):
                assert t.device.index in (None, self.device), f"{name}: on device {t.device.index}, the raytracer is on {self.device}"
        except AssertionError as e:
            raise ValueError(f"set_triangles_from: {e}") from None
        _call("rrt_raytracer_set_triangles_device", self._h, n, _ptr(pos_t), _ptr(uv_t), _ptr(nrm_t), _ptr(mat_t), _root(root), _P(_stream(stream)))

    def release_update_memory(self) -> None:
        """rrt_raytracer_release_update_memory: frees the device memory kept between set_triangles calls (the next one allocates again)."""
        _call("rrt_raytracer_release_update_memory", self._h)

    # raytracer.rs:29, batched
    def get_ray_colours(self, origins, dirs) -> np.ndarray:
        o, d, _ = _host_rays(origins, dirs)
        out = np.empty(o.shape[0], np.uint32)
        _call("rrt_get_ray_colours", self._h, o.shape[0], _d(o), _d(d), _u32(out))
        return out

    def get_ray_colour(self, origin: Vector3d, direction: Vector3d) -> int:
        return int(self.get_ray_colours([[origin.x, origin.y, origin.z]], [[direction.x, direction.y, direction.z]])[0])

    # ray.rs:96-168, batched
    def intersect_rays(self, origins, dirs, max_t=None):
        o, d, mt = _host_rays(origins, dirs, max_t)
        n = o.shape[0]
        hit = np.empty(n, np.uint8); t = np.empty(n); u = np.empty(n); v = np.empty(n); tri = np.empty(n, np.uint32)
        _call("rrt_intersect_rays", self._h, n, _d(o), _d(d), _d(mt), _u8(hit), _d(t), _d(u), _d(v), _u32(tri))
        return hit.astype(bool), t, u, v, tri

    # Some/None of the same walk (rrt.h: rrt_occluded_rays): the reference's shadow query without its negation
    def occluded(self, origins, dirs, max_t=None) -> np.ndarray:
        o, d, mt = _host_rays(origins, dirs, max_t)
        out = np.empty(o.shape[0], np.uint8)
        _call("rrt_occluded_rays", self._h, o.shape[0], _d(o), _d(d), _d(mt), _u8(out))
        return out.astype(bool)

    # device-resident ray batches (rrt.h: rrt_intersect_rays_device): origins_t / dirs_t are float64 device tensors of 3 n elements, max_t_t of n; enqueued, not synchronised
    # bound_t, in all ten _into forms that have it: None, or a device tensor of one 4-byte element -- the launch bound of the counted form (rrt.h: COUNTED DEVICE
    # FORMS), read on the device in stream order: only the first min(n, bound) entries of every array are read and written.
    def occluded_into(self, origins_t, dirs_t, out_t, max_t_t=None, stream: Optional[int] = None, bound_t=None):
        """rrt_occluded_rays_device: out_t = device tensor of n one-byte elements, 1 = occluded.  bound_t: rrt_occluded_rays_counted_device."""
        n = _ray_batch(origins_t, dirs_t, max_t_t)
        _device_tensor(out_t, n, 1, "out")
        _call(*_bounded("rrt_occluded_rays_device", bound_t, self._h, n), _ptr(origins_t), _ptr(dirs_t), _ptr(max_t_t), _ptr(out_t), _P(_stream(stream)))

    def intersect_rays_into(self, origins_t, dirs_t, out: dict, max_t_t=None, stream: Optional[int] = None, bound_t=None):
        """rrt_intersect_rays_device: out = {name: device tensor of n elements} for any subset of hit (1 byte), t, u, v (float64), tri (4 bytes); the others are not
        computed.  bound_t: rrt_intersect_rays_counted_device."""
        n = _ray_batch(origins_t, dirs_t, max_t_t)
        assert set(out) <= set(PLANES[:5]), sorted(out)
        for name, t in out.items():
            _device_tensor(t, n, np.dtype(PLANE_DTYPES[name]).itemsize, name)
        _call(*_bounded("rrt_intersect_rays_device", bound_t, self._h, n), _ptr(origins_t), _ptr(dirs_t), _ptr(max_t_t), *(_ptr(out.get(name)) for name in PLANES[:5]),
              _P(_stream(stream)))

    def get_ray_colours_into(self, origins_t, dirs_t, colours_t, stream: Optional[int] = None, bound_t=None):
        """rrt_get_ray_colours_device: colours_t = device tensor of n four-byte elements, 0x00RRGGBB.  bound_t: rrt_get_ray_colours_counted_device."""
        n = _ray_batch(origins_t, dirs_t, None)
        _device_tensor(colours_t, n, 4, "colours")
        _call(*_bounded("rrt_get_ray_colours_device", bound_t, self._h, n), _ptr(origins_t), _ptr(dirs_t), _ptr(colours_t), _P(_stream(stream)))

    def tune_rays(self, origins_t, dirs_t, max_t_t=None) -> int:
        """rrt_tune_rays_device (blocking): measures the three traversal variants on this device-resident batch and keeps the fastest for later per-ray calls;
        returns it (an index into VARIANT_NAMES).  The current torch stream is synchronised first: the measurement runs on the default stream."""
        n = _ray_batch(origins_t, dirs_t, max_t_t)
        import torch
        torch.cuda.current_stream().synchronize()
        v = C.c_uint32(0)
        _call("rrt_tune_rays_device", self._h, n, _ptr(origins_t), _ptr(dirs_t), _ptr(max_t_t), C.byref(v))
        return int(v.value)

    # the surface record of arbitrary rays (rrt.h: rrt_surface_rays): what surface() gives for the frame's primary rays, for the caller's own, and the next ray
    def surface_rays(self, origins, dirs, max_t=None, planes=RAY_SURFACE_PLANES) -> dict:
        """rrt_surface_rays: {name: array} for the names asked for, from RAY_SURFACE_PLANES: hit uint8, t / u / v float64, tri / albedo / material / lights uint32
        [n]; point / normal / next_origin / next_dir float64 [n][3] (next_*: the reference's reflection ray from the hit).  A ray with a NaN or non-positive
        max_t is a miss in every array."""
        o, d, mt = _host_rays(origins, dirs, max_t)
        n = o.shape[0]
        out = {name: np.empty((n, width) if width > 1 else (n,), dtype) for name, (dtype, width) in ((name, _ray_plane(name)) for name in planes)}
        _call("rrt_surface_rays", self._h, n, _d(o), _d(d), _d(mt), _plane_struct(CRaySurface, out))
        return out

    def surface_rays_into(self, origins_t, dirs_t, out: dict, max_t_t=None, stream: Optional[int] = None, bound_t=None):
        """rrt_surface_rays_device: out = {name: contiguous device tensor} for any subset of RAY_SURFACE_PLANES -- n elements of the array's item size, 3 n for
        point / normal / next_origin / next_dir; the others are not computed.  Enqueued, not synchronised.  bound_t: rrt_surface_rays_counted_device."""
        n = _ray_batch(origins_t, dirs_t, max_t_t)
        for name, t in out.items():
            dtype, width = _ray_plane(name)
            _device_tensor(t, width * n, np.dtype(dtype).itemsize, name)
        _call(*_bounded("rrt_surface_rays_device", bound_t, self._h, n), _ptr(origins_t), _ptr(dirs_t), _ptr(max_t_t), _plane_struct(CRaySurface, out), _P(_stream(stream)))

    # shading of arbitrary rays from kept records (rrt.h: rrt_shade_rays): what shade() does for a frame's planes, for the arrays surface_rays wrote
    def shade_rays(self, dirs, planes: dict, depth: int = 0, outputs=("colour",)) -> dict:
        """rrt_shade_rays: {name: array} for the names asked for, from RAY_SHADE_OUTPUTS -- colour uint32 [n] 0x00RRGGBB, local float64 [n][3] (the unquantised
        local colour), kr float64 [n] -- of the rays with the directions `dirs` whose records `planes` holds ({name: array} as surface_rays returns it: albedo,
        point, normal and material are read, lights if it is there; the others are ignored), with the lights and materials in force now.  depth: the recursion
        depth at which the batch stands.  With depth 0 and the records surface_rays wrote for (origins, dirs), colour is get_ray_colours(origins, dirs)."""
        d = np.ascontiguousarray(dirs, np.float64).reshape(-1, 3)
        n = d.shape[0]
        rec = {name: np.ascontiguousarray(a, dtype) for name, (a, dtype, width) in _ray_records("shade_rays", planes).items()}
        for name, a in rec.items():
            assert a.size == n * _ray_plane(name)[1], f"shade_rays: array {name} has {a.size} elements for {n} rays"
        out = {name: np.empty((n, width) if width > 1 else (n,), dtype) for name, (dtype, width) in ((name, _ray_plane(name, CRayShade, "shade_rays")) for name in outputs)}
        _call("rrt_shade_rays", self._h, n, _d(d), _plane_struct(CRaySurface, rec), int(depth), _plane_struct(CRayShade, out))
        return out

    def shade_rays_into(self, out: dict, dirs_t, planes: dict, depth: int = 0, stream: Optional[int] = None, bound_t=None):
        """rrt_shade_rays_device: out = {name: contiguous device tensor} for any subset of RAY_SHADE_OUTPUTS (n four-byte elements, 3 n and n float64; the others
        are not computed -- without colour no reflection ray is walked); dirs_t float64 of 3 n elements; planes = {name: device tensor} as surface_rays_into
        filled them (albedo, point, normal, material, and lights or not).  Enqueued, not synchronised.  bound_t: rrt_shade_rays_counted_device."""
        n = _batch_size(dirs_t, 3, "dirs")
        _device_tensor(dirs_t, 3 * n, 8, "dirs")
        rec = _ray_records("shade_rays_into", planes)
        for name, (t, dtype, width) in rec.items():
            _device_tensor(t, width * n, np.dtype(dtype).itemsize, name)
        for name, t in out.items():
            dtype, width = _ray_plane(name, CRayShade, "shade_rays_into")
            _device_tensor(t, width * n, np.dtype(dtype).itemsize, name)
        _call(*_bounded("rrt_shade_rays_device", bound_t, self._h, n), _ptr(dirs_t), _plane_struct(CRaySurface, {name: row[0] for name, row in rec.items()}), int(depth),
              _plane_struct(CRayShade, out), _P(_stream(stream)))

    # ambient occlusion for ray records (rrt.h: rrt_ambient_rays): what ambient() does for a frame's planes, for the arrays surface_rays wrote, with a rotation per record
    def ambient_rays(self, planes: dict, dirs, max_t: float = float("inf"), rot=None, outputs=RAY_AMBIENT_OUTPUTS) -> dict:
        """rrt_ambient_rays: {name: array} for the names asked for, from RAY_AMBIENT_OUTPUTS -- occluded uint32 [n], bit k = ray k of the record's fan is blocked;
        open uint32 [n], the number of open rays (all of them for a miss) -- of the records `planes` holds ({name: array} as surface_rays returns it: point, normal
        and material are read; the others are ignored).  dirs: [n_samples][3] directions in the tangent frame of a hit, as ambient() takes them; rot: None or
        [n][2] float64, (cos, sin) of the angle by which each record's fan is turned about its normal."""
        rec = {name: np.ascontiguousarray(a, dtype) for name, (a, dtype, width) in _ray_records("ambient_rays", planes, RAY_AMBIENT_INPUTS).items()}
        assert "material" in rec, "ambient_rays: the records have no material array"
        n = rec["material"].size
        for name, a in rec.items():
            assert a.size == n * _ray_plane(name)[1], f"ambient_rays: array {name} has {a.size} elements for {n} rays"
        r = None if rot is None else np.ascontiguousarray(rot, np.float64)
        assert r is None or r.size == 2 * n, f"ambient_rays: rot has {r.size} elements for {n} rays"
        _d_keep, samples = _ambient_samples(dirs, max_t)
        out = {name: np.empty(n, dtype) for name, (dtype, width) in ((name, _ray_plane(name, CRayAmbient, "ambient_rays")) for name in outputs)}
        _call("rrt_ambient_rays", self._h, n, _plane_struct(CRaySurface, rec), _d(r), C.byref(samples), _plane_struct(CRayAmbient, out))
        return out

    def ambient_rays_into(self, out: dict, planes: dict, dirs, max_t: float, rot_t=None, stream: Optional[int] = None, bound_t=None):
        """rrt_ambient_rays_device: out = {name: contiguous device tensor of n four-byte elements} for any subset of RAY_AMBIENT_OUTPUTS; planes = {name: device
        tensor} as surface_rays_into filled them (point, normal, material); rot_t None or a float64 device tensor of 2 n elements.  The sample table `dirs` is a
        host array.  Enqueued, not synchronised.  bound_t: rrt_ambient_rays_counted_device."""
        rec = _ray_records("ambient_rays_into", planes, RAY_AMBIENT_INPUTS)
        assert "material" in rec, "ambient_rays_into: the records have no material array"
        n = _batch_size(rec["material"][0], 1, "material")
        for name, (t, dtype, width) in rec.items():
            _device_tensor(t, width * n, np.dtype(dtype).itemsize, name)
        if rot_t is not None:
            _device_tensor(rot_t, 2 * n, 8, "rot")
        for name, t in out.items():
            dtype, width = _ray_plane(name, CRayAmbient, "ambient_rays_into")
            _device_tensor(t, width * n, np.dtype(dtype).itemsize, name)
        _d_keep, samples = _ambient_samples(dirs, max_t)
        _call(*_bounded("rrt_ambient_rays_device", bound_t, self._h, n), _plane_struct(CRaySurface, {name: row[0] for name, row in rec.items()}), _ptr(rot_t), C.byref(samples),
              _plane_struct(CRayAmbient, out), _P(_stream(stream)))

    # surface records from kept hits (rrt.h: rrt_resolve_hits): what surface_rays gives, from the t, u, v and tri an earlier walk of the rays left, with no primary walk
    def resolve_hits(self, origins, dirs, planes: dict, outputs=RESOLVE_OUTPUTS) -> dict:
        """rrt_resolve_hits: {name: array} for the names asked for, from RESOLVE_OUTPUTS -- as surface_rays returns them -- of the rays (origins, dirs) whose kept
        hits `planes` holds ({name: array} as intersect_rays, surface_rays or visibility wrote them: t and tri are read, u and v unless only point and / or material
        are asked for; the others are ignored), with the lights and materials in force now.  An entry whose tri is not a triangle of the scene is a miss."""
        o, d, _ = _host_rays(origins, dirs)
        n = o.shape[0]
        rec = {name: np.ascontiguousarray(a, dtype) for name, (a, dtype, width) in _ray_records("resolve_hits", planes, RESOLVE_INPUTS).items()}
        for name, a in rec.items():
            assert a.size == n, f"resolve_hits: array {name} has {a.size} elements for {n} rays"
        out = {name: np.empty((n, width) if width > 1 else (n,), dtype) for name, (dtype, width) in ((name, _resolve_output(name, "resolve_hits")) for name in outputs)}
        _call("rrt_resolve_hits", self._h, n, _d(o), _d(d), _plane_struct(CRaySurface, {**rec, **out}))
        return out

    def resolve_hits_into(self, out: dict, origins_t, dirs_t, planes: dict, stream: Optional[int] = None, bound_t=None):
        """rrt_resolve_hits_device: out = {name: contiguous device tensor} for any subset of RESOLVE_OUTPUTS (n elements of the array's item size, 3 n for point /
        normal / next_origin / next_dir; the others are not computed -- without lights nothing is walked); origins_t / dirs_t float64 of 3 n elements; planes =
        {name: device tensor} as intersect_rays_into or surface_rays_into filled them (t, tri, and u, v or not).  Enqueued, not synchronised.  bound_t:
        rrt_resolve_hits_counted_device."""
        n = _ray_batch(origins_t, dirs_t, None)
        rec = _ray_records("resolve_hits_into", planes, RESOLVE_INPUTS)
        for name, (t, dtype, width) in rec.items():
            _device_tensor(t, width * n, np.dtype(dtype).itemsize, name)
        for name, t in out.items():
            dtype, width = _resolve_output(name, "resolve_hits_into")
            _device_tensor(t, width * n, np.dtype(dtype).itemsize, name)
        _call(*_bounded("rrt_resolve_hits_device", bound_t, self._h, n), _ptr(origins_t), _ptr(dirs_t),
              _plane_struct(CRaySurface, {**{name: row[0] for name, row in rec.items()}, **out}), _P(_stream(stream)))

    # compaction of ray batches and records, and its inverse (rrt.h: rrt_compact_rays, rrt_scatter_rays): the survivors to the front of a batch that keeps its length
    def compact_rays(self, planes: dict, select: str = "hit", flag=None, origins=None, dirs=None, max_t=None, rot=None) -> dict:
        """rrt_compact_rays: {"index": uint32 [n], "count": int, name: the gathered array} for every array given -- `planes` ({name: array} as surface_rays
        returns it, any of RAY_SURFACE_PLANES; may be empty) and origins / dirs [n][3], max_t [n], rot [n][2].  select: "hit" (material < n_mats), "mirror" (and
        kr > 0 in the table in force) or "flag" (flag[i] != 0, uint8 [n]).  The survivors come first, in their order; the tail holds dead entries (max_t NaN,
        material 0xFFFFFFFF, rrt.h) and index DEAD_INDEX.  max_t=True: no bound is read, the survivors get +inf."""
        sel = _select(select, "compact_rays")
        src = {name: np.ascontiguousarray(a, dtype) for name, (a, dtype, width) in _ray_records("compact_rays", planes, RAY_SURFACE_PLANES).items()}
        for name, a in (("origins", origins), ("dirs", dirs), ("max_t", max_t), ("rot", rot)):
            if a is not None and a is not True:
                src[name] = np.ascontiguousarray(a, np.float64)
        f = None if flag is None else np.ascontiguousarray(flag, np.uint8)
        lead = f if sel == 2 else src.get("material")
        assert lead is not None, f"compact_rays: select {select!r} needs {'a flag array' if sel == 2 else 'a material array'}"
        n = lead.size
        assert f is None or f.size == n, f"compact_rays: flag has {f.size} elements for {n} entries"
        for name, a in src.items():
            assert a.size == n * _ray_plane(name, CRaySet, "compact_rays")[1], f"compact_rays: array {name} has {a.size} elements for {n} entries"
        out = {name: np.empty_like(a) for name, a in src.items()}
        if max_t is True:
            out["max_t"] = np.empty(n, np.float64)
        index, count = np.empty(n, np.uint32), C.c_uint32(0)
        _call("rrt_compact_rays", self._h, n, sel, _u8(f), _ray_set(src), _ray_set(out), _u32(index), C.byref(count))
        return dict(out, index=index, count=int(count.value))

    def compact_rays_into(self, out: dict, src: dict, select: str, index_t, count_t, scratch_t, flag_t=None, stream: Optional[int] = None, bound_t=None):
        """rrt_compact_rays_device: out / src = {name: contiguous device tensor} with names from RAY_SET_ARRAYS -- n elements of the array's item size, 3 n for the
        vectors, 2 n for rot; every array of out but max_t needs its array of src.  index_t: n four-byte elements or None; count_t: one four-byte element or None;
        scratch_t: a device tensor of at least compact_scratch_bytes(n) bytes (None for n == 0); flag_t: n bytes, for select "flag".  n is the length of flag_t
        for "flag", of src["material"] otherwise.  Enqueued, not synchronised; last_stats stays as it was.  bound_t: rrt_compact_rays_counted_device (count_t is the
        OUTPUT count; the two must not be the same word)."""
        sel = _select(select, "compact_rays_into")
        lead = flag_t if sel == 2 else src.get("material")
        assert lead is not None, f"compact_rays_into: select {select!r} needs {'a flag tensor' if sel == 2 else 'a material tensor'}"
        n = _batch_size(lead, 1, "flag" if sel == 2 else "material")
        if flag_t is not None:
            _device_tensor(flag_t, n, 1, "flag")
        for what, arrays in (("src", src), ("out", out)):
            for name, t in arrays.items():
                dtype, width = _ray_plane(name, CRaySet, "compact_rays_into")
                _device_tensor(t, width * n, np.dtype(dtype).itemsize, f"{what} {name}")
        if index_t is not None:
            _device_tensor(index_t, n, 4, "index")
        if count_t is not None:
            _device_tensor(count_t, 1, 4, "count")
        scratch_bytes = 0
        if scratch_t is not None:
            assert getattr(scratch_t, "is_cuda", False) and scratch_t.is_contiguous(), "scratch: not a contiguous device tensor"
            scratch_bytes = scratch_t.numel() * scratch_t.element_size()
        _call(*_bounded("rrt_compact_rays_device", bound_t, self._h, n), sel, _ptr(flag_t), _ray_set(src), _ray_set(out), _ptr(index_t), _ptr(count_t), _ptr(scratch_t),
              scratch_bytes, _P(_stream(stream)))

    def scatter_rays(self, index, src, dst) -> np.ndarray:
        """rrt_scatter_rays: dst[index[j]] = src[j] for every j with index[j] < n; index uint32 [n], src and dst arrays of n elements of 1, 4, 8, 16 or 24 bytes
        (dst: a contiguous, writable array of src's dtype, written in place and returned; elements no j names stay)."""
        idx = np.ascontiguousarray(index, np.uint32).reshape(-1)
        n = idx.size
        assert isinstance(dst, np.ndarray) and dst.flags.c_contiguous and dst.flags.writeable, "scatter_rays: dst is not a contiguous writable array"
        s = np.ascontiguousarray(src, dst.dtype)
        assert s.size == dst.size and s.nbytes == dst.nbytes and (n == 0 or s.nbytes % n == 0), f"scatter_rays: src has {s.size} elements and dst {dst.size} for {n} entries"
        _call("rrt_scatter_rays", self._h, n, _u32(idx), s.nbytes // n if n else s.itemsize, _P(s.ctypes.data), _P(dst.ctypes.data))
        return dst

    def scatter_rays_into(self, index_t, src_t, dst_t, stream: Optional[int] = None, bound_t=None):
        """rrt_scatter_rays_device: index_t n four-byte elements, src_t and dst_t contiguous device tensors of n elements of 1, 4, 8, 16 or 24 bytes (k n elements
        of a k-wide array).  Enqueued, not synchronised.  bound_t: rrt_scatter_rays_counted_device."""
        n = _batch_size(index_t, 1, "index")
        _device_tensor(index_t, n, 4, "index")
        assert getattr(src_t, "is_cuda", False), "src: not a device tensor"
        per, rem = divmod(src_t.numel(), n) if n else (1, 0)
        assert rem == 0 and per >= 1, f"src: {src_t.numel()} elements for {n} entries"
        _device_tensor(src_t, per * n, src_t.element_size(), "src")
        _device_tensor(dst_t, per * n, src_t.element_size(), "dst")
        _call(*_bounded("rrt_scatter_rays_device", bound_t, self._h, n), _ptr(index_t), per * src_t.element_size(), _ptr(src_t), _ptr(dst_t), _P(_stream(stream)))

    compact_scratch_bytes = staticmethod(compact_scratch_bytes)

    # stable sort of ray batches and records by a coherence key (rrt.h: rrt_sort_rays): entries that start in the same cell and head the same way become neighbours
    def sort_rays(self, planes: dict, key: str = "ray", keys=None, origins=None, dirs=None, max_t=None, rot=None) -> dict:
        """rrt_sort_rays: {"index": uint32 [n], "keys": uint32 [n] (sorted), "count": int, name: the gathered array} for every array given -- `planes` ({name:
        array} as surface_rays returns it, any of RAY_SURFACE_PLANES; may be empty) and origins / dirs [n][3], max_t [n], rot [n][2].  key: "given" (keys, uint32
        [n]), "ray" (origins and dirs; dead where max_t is not above 0) or "record" (point and normal; dead where material is no material).  Ascending and stable;
        dead entries (key DEAD_KEY) form the tail, in source order, and are gathered like the rest."""
        mode = _key_mode(key, "sort_rays")
        src = {name: np.ascontiguousarray(a, dtype) for name, (a, dtype, width) in _ray_records("sort_rays", planes, RAY_SURFACE_PLANES).items()}
        for name, a in (("origins", origins), ("dirs", dirs), ("max_t", max_t), ("rot", rot)):
            if a is not None:
                src[name] = np.ascontiguousarray(a, np.float64)
        k = None if keys is None else np.ascontiguousarray(keys, np.uint32)
        for name in _SORT_KEY_READS[mode]:
            assert name in src, f"sort_rays: key {key!r} needs the array {name}"
        assert mode != 0 or k is not None, "sort_rays: key 'given' needs a keys array"
        n = k.size if mode == 0 else src["origins"].size // 3 if mode == 1 else src["material"].size
        assert k is None or k.size == n, f"sort_rays: keys has {k.size} elements for {n} entries"
        for name, a in src.items():
            assert a.size == n * _ray_plane(name, CRaySet, "sort_rays")[1], f"sort_rays: array {name} has {a.size} elements for {n} entries"
        out = {name: np.empty_like(a) for name, a in src.items()}
        index, keys_out, count = np.empty(n, np.uint32), np.empty(n, np.uint32), C.c_uint32(0)
        _call("rrt_sort_rays", self._h, n, mode, _u32(k), _ray_set(src), _ray_set(out), _u32(index), _u32(keys_out), C.byref(count))
        return dict(out, index=index, keys=keys_out, count=int(count.value))

    def sort_rays_into(self, out: dict, src: dict, key: str, index_t, keys_out_t, count_t, scratch_t, keys_t=None, stream: Optional[int] = None):
        """rrt_sort_rays_device: out / src = {name: contiguous device tensor} with names from RAY_SET_ARRAYS -- n elements of the array's item size, 3 n for the
        vectors, 2 n for rot; every array of out needs its array of src.  index_t, keys_out_t: n four-byte elements or None; count_t: one four-byte element or
        None; scratch_t: a device tensor of at least sort_scratch_bytes(n) bytes (None for n == 0); keys_t: n four-byte elements, for key "given".  n is the length
        of keys_t for "given", of src["origins"] for "ray", of src["material"] for "record".  Enqueued, not synchronised; last_stats stays as it was."""
        mode = _key_mode(key, "sort_rays_into")
        for name in _SORT_KEY_READS[mode]:
            assert src.get(name) is not None, f"sort_rays_into: key {key!r} needs the tensor {name}"
        assert mode != 0 or keys_t is not None, "sort_rays_into: key 'given' needs a keys tensor"
        n = _batch_size(keys_t, 1, "keys") if mode == 0 else _batch_size(src["origins"], 3, "origins") if mode == 1 else _batch_size(src["material"], 1, "material")
        if keys_t is not None:
            _device_tensor(keys_t, n, 4, "keys")
        for what, arrays in (("src", src), ("out", out)):
            for name, t in arrays.items():
                dtype, width = _ray_plane(name, CRaySet, "sort_rays_into")
                _device_tensor(t, width * n, np.dtype(dtype).itemsize, f"{what} {name}")
        for name, t, size in (("index", index_t, n), ("keys_out", keys_out_t, n), ("count", count_t, 1)):
            if t is not None:
                _device_tensor(t, size, 4, name)
        scratch_bytes = 0
        if scratch_t is not None:
            assert getattr(scratch_t, "is_cuda", False) and scratch_t.is_contiguous(), "scratch: not a contiguous device tensor"
            scratch_bytes = scratch_t.numel() * scratch_t.element_size()
        _call("rrt_sort_rays_device", self._h, n, mode, _ptr(keys_t), _ray_set(src), _ray_set(out), _ptr(index_t), _ptr(keys_out_t), _ptr(count_t), _ptr(scratch_t),
              scratch_bytes, _P(_stream(stream)))

    sort_scratch_bytes = staticmethod(sort_scratch_bytes)

    # the two ends of the per-ray pipeline (rrt.h: rrt_frame_rays, rrt_mix_rays, rrt_mix_pixels) and the frame by ray generations (rrt_render_wavefront)
    frame_ray_count = staticmethod(frame_ray_count)

    def frame_rays(self, width: int, height: int, region=None, order: int = ORDER_ROWS, arrays=FRAME_RAY_ARRAYS) -> dict:
        """rrt_frame_rays: {name: array} for the names asked for, from FRAME_RAY_ARRAYS -- origins, dirs float64 [n][3], max_t float64 [n] -- of the primary rays a
        frame traces in the region in the pose in force, n = frame_ray_count(...).  A dead entry (a pixel the reference never traces; in tiles order a pixel outside
        the region) has a zero origin and direction and max_t NaN."""
        reg, o = _region(width, height, region)[0], _order(order, "frame_rays")
        n = frame_ray_count(width, height, region, o)
        out = {name: np.empty((n, w) if w > 1 else (n,), dtype) for name, (dtype, w) in ((name, _frame_ray_array(name, "frame_rays")) for name in arrays)}
        _call("rrt_frame_rays", self._h, width, height, reg, o, *(_d(out.get(name)) for name in FRAME_RAY_ARRAYS))
        return out

    def frame_rays_into(self, out: dict, width: int, height: int, region=None, order: int = ORDER_ROWS, stream: Optional[int] = None):
        """rrt_frame_rays_device: out = {name: contiguous float64 device tensor} for any subset of FRAME_RAY_ARRAYS -- 3 n elements for origins and dirs, n for max_t,
        n = frame_ray_count(...).  Enqueued, not synchronised; last_stats stays as it was."""
        reg, o = _region(width, height, region)[0], _order(order, "frame_rays_into")
        n = frame_ray_count(width, height, region, o)
        for name, t in out.items():
            dtype, w = _frame_ray_array(name, "frame_rays_into")
            _device_tensor(t, w * n, np.dtype(dtype).itemsize, name)
        _call("rrt_frame_rays_device", self._h, width, height, reg, o, *(_ptr(out.get(name)) for name in FRAME_RAY_ARRAYS), _P(_stream(stream)))

    def mix_rays(self, local, kr=None, reflected=None, material=None) -> np.ndarray:
        """rrt_mix_rays: colour uint32 [n] of one level of the unwind -- 0x00FFFFFF where material is no material, the clamped `local` (float64 [n][3]) where
        kr (float64 [n]) is not above 0 or kr or reflected is None, local * (1 - kr) + reflected * kr per channel, clamped, elsewhere.  reflected: uint32 [n], the
        colours of the level below in this level's order.  material None: every entry is a hit."""
        l = np.ascontiguousarray(local, np.float64).reshape(-1, 3)
        n = l.shape[0]
        k, r, m = (None if a is None else np.ascontiguousarray(a, dtype).reshape(-1) for a, dtype in ((kr, np.float64), (reflected, np.uint32), (material, np.uint32)))
        for name, a in (("kr", k), ("reflected", r), ("material", m)):
            assert a is None or a.size == n, f"mix_rays: {name} has {a.size} elements for {n} entries"
        colour = np.empty(n, np.uint32)
        _call("rrt_mix_rays", self._h, n, _u32(m), _d(l), _d(k), _u32(r), _u32(colour))
        return colour

    def mix_rays_into(self, colour_t, local_t, kr_t=None, reflected_t=None, material_t=None, stream: Optional[int] = None, bound_t=None):
        """rrt_mix_rays_device: colour_t n four-byte elements; local_t float64 of 3 n elements; kr_t float64 of n, reflected_t and material_t n four-byte elements,
        each or None.  Enqueued, not synchronised; last_stats stays as it was.  bound_t: rrt_mix_rays_counted_device."""
        n = _batch_size(local_t, 3, "local")
        _device_tensor(local_t, 3 * n, 8, "local"); _device_tensor(colour_t, n, 4, "colour")
        for name, t, size in (("kr", kr_t, 8), ("reflected", reflected_t, 4), ("material", material_t, 4)):
            if t is not None:
                _device_tensor(t, n, size, name)
        _call(*_bounded("rrt_mix_rays_device", bound_t, self._h, n), _ptr(material_t), _ptr(local_t), _ptr(kr_t), _ptr(reflected_t), _ptr(colour_t), _P(_stream(stream)))

    def mix_pixels(self, colours, width: int, height: int, region=None, order: int = ORDER_ROWS) -> np.ndarray:
        """rrt_mix_pixels: the region's pixels, [h][w] uint32 0x00RRGGBB, from the colours of its ray batch (uint32, frame_ray_count(...) of them, in `order`):
        Color::mix of a pixel's four sub-samples, 0 for a pixel the reference never traces."""
        reg, w, h = _region(width, height, region)
        o = _order(order, "mix_pixels")
        c = np.ascontiguousarray(colours, np.uint32).reshape(-1)
        n = frame_ray_count(width, height, region, o)
        assert c.size == n, f"mix_pixels: colours has {c.size} elements for {n} entries"
        fb = np.empty((h, w), np.uint32)
        _call("rrt_mix_pixels", self._h, width, height, reg, o, _u32(c), _u32(fb))
        return fb

    def mix_pixels_into(self, fb_tensor, colours_t, width: int, height: int, region=None, order: int = ORDER_ROWS, stream: Optional[int] = None):
        """rrt_mix_pixels_device: colours_t = frame_ray_count(...) four-byte elements in `order`; fb_tensor = w*h four-byte elements of the region.  Enqueued, not
        synchronised; last_stats stays as it was."""
        reg, w, h = _region(width, height, region)
        o = _order(order, "mix_pixels_into")
        _device_tensor(colours_t, frame_ray_count(width, height, region, o), 4, "colours")
        _device_tensor(fb_tensor, w * h, 4, "fb")
        _call("rrt_mix_pixels_device", self._h, width, height, reg, o, _ptr(colours_t), _ptr(fb_tensor), _P(_stream(stream)))

    def wavefront_work_bytes(self, width: int, height: int, region=None, order: int = ORDER_ROWS) -> int:
        """rrt_wavefront_work_bytes: the device work memory render_wavefront_into needs for this region and order; 0 for arguments the library refuses."""
        return int(lib().rrt_wavefront_work_bytes(self._h, int(width), int(height), _region(width, height, region)[0], _order(order, "wavefront_work_bytes")))

    def render_wavefront(self, width: int, height: int, region=None, order: int = ORDER_ROWS) -> np.ndarray:
        """rrt_render_wavefront: the region of the frame render() produces, [h][w] uint32, traced as compacted ray generations -- frame rays, then per reflection
        level surface records, local and kr, compaction of the mirror hits; the unwind back up; the pixels."""
        reg, w, h = _region(width, height, region)
        fb = np.empty((h, w), np.uint32)
        _call("rrt_render_wavefront", self._h, width, height, reg, _order(order, "render_wavefront"), _u32(fb))
        return fb

    def render_wavefront_into(self, fb_tensor, work_t, width: int, height: int, region=None, order: int = ORDER_ROWS, stream: Optional[int] = None):
        """rrt_render_wavefront_device: fb_tensor = w*h four-byte elements of the region; work_t = a contiguous device tensor of at least
        wavefront_work_bytes(...) bytes, 256-byte aligned, whose contents mean nothing.  Enqueued, not synchronised."""
        reg, w, h = _region(width, height, region)
        o = _order(order, "render_wavefront_into")
        _device_tensor(fb_tensor, w * h, 4, "fb")
        assert getattr(work_t, "is_cuda", False) and work_t.is_contiguous(), "work: not a contiguous device tensor"
        _call("rrt_render_wavefront_device", self._h, width, height, reg, o, _ptr(fb_tensor), _ptr(work_t), work_t.numel() * work_t.element_size(), _P(_stream(stream)))

    # engine.rs:196-253: chunked draw with an update after every chunk (on_update(fb, first_row, n_rows) stands in for canvas.update())
    def render_progressive(self, width: int, height: int, on_update=None, chunk_rows: int = 50) -> np.ndarray:
        fb = np.empty((height, width), np.uint32)
        UPD = C.CFUNCTYPE(None, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32)
        cb = UPD(lambda user, p, w, h, r0, n: on_update(fb, int(r0), int(n))) if on_update is not None else None
        _call("rrt_render_progressive", self._h, width, height, _u32(fb), chunk_rows, C.cast(cb, _P) if cb is not None else None, None)
        return fb

    # engine.rs:186 via the C ABI, host framebuffer
    def render(self, width: int, height: int) -> np.ndarray:
        fb = np.empty((height, width), np.uint32)
        _call("rrt_render", self._h, width, height, _u32(fb))
        return fb

    def render_registered(self, width: int, height: int, fb: Optional[np.ndarray] = None) -> np.ndarray:
        """rrt_render into a page-locked framebuffer (rrt_host_buffer_register): the frame arrives by one asynchronous DMA."""
        if fb is None:
            fb = np.empty((height, width), np.uint32)
        p = _P(fb.ctypes.data)
        _call("rrt_host_buffer_register", p, fb.nbytes)
        try:
            _call("rrt_render", self._h, width, height, _u32(fb))
        finally:
            _call("rrt_host_buffer_unregister", p)
        return fb

    # device-resident variants (torch tensors are plumbing: data_ptr + current stream)
    def render_into(self, fb_tensor, width: int, height: int, stream: Optional[int] = None):
        self.bind_render(fb_tensor, width, height, stream)()

    def render_tiles_into(self, tiles_tensor, width: int, height: int, rank: int, world: int, stream: Optional[int] = None):
        self.bind_render_tiles(tiles_tensor, width, height, rank, world, stream)()

    def detile_into(self, gathered_tensor, fb_tensor, width: int, height: int, world: int, stream: Optional[int] = None):
        self.bind_detile(gathered_tensor, fb_tensor, width, height, world, stream)()

    # pre-bound launchers for per-frame loops (bench.py): all argument conversion is done once, the returned callable is one ctypes call
    def bind_render(self, fb_tensor, width: int, height: int, stream: Optional[int] = None):
        _device_tensor(fb_tensor, width * height, 4, "fb")
        return _bound("rrt_render_device", self._h, C.c_uint32(width), C.c_uint32(height), _ptr(fb_tensor), _P(_stream(stream)))

    def bind_render_tiles(self, tiles_tensor, width: int, height: int, rank: int, world: int, stream: Optional[int] = None):
        _device_tensor(tiles_tensor, tiles_per_rank(width, height, world) * 64, 4, "tiles")
        return _bound("rrt_render_tiles_device", self._h, C.c_uint32(width), C.c_uint32(height), C.c_uint32(rank), C.c_uint32(world), _ptr(tiles_tensor),
                      _P(_stream(stream)))

    def bind_detile(self, gathered_tensor, fb_tensor, width: int, height: int, world: int, stream: Optional[int] = None):
        _device_tensor(gathered_tensor, tiles_per_rank(width, height, world) * 64 * world, 4, "gathered")
        _device_tensor(fb_tensor, width * height, 4, "fb")
        return _bound("rrt_detile_device", self._h, C.c_uint32(width), C.c_uint32(height), C.c_uint32(world), _ptr(gathered_tensor), _ptr(fb_tensor),
                      _P(_stream(stream)))

    # the fused frame of a region and of a device-resident tile list (rrt.h: rrt_render_region, rrt_render_tile_list_device): the pixels render() gives, by the same kernel body
    def render_region(self, width: int, height: int, region=None) -> np.ndarray:
        """rrt_render_region: the region's pixels, [h][w] uint32 0x00RRGGBB: render(width, height)[y0:y0+h, x0:x0+w] bit for bit, traced for the region alone."""
        reg, w, h = _region(width, height, region)
        fb = np.empty((h, w), np.uint32)
        _call("rrt_render_region", self._h, width, height, reg, _u32(fb), 0)
        return fb

    def render_region_into(self, fb_tensor, width: int, height: int, region=None, pitch: Optional[int] = None, offset: int = 0, stream: Optional[int] = None):
        """rrt_render_region_device: the region's pixels into rows of `pitch` four-byte elements (None: the region's width, a tight [h][w] array) that begin `offset`
        elements into fb_tensor, a contiguous device tensor that holds all of them; nothing else of it is touched.  With fb_tensor a whole [height][width] frame,
        pitch = width and offset = y0 * width + x0 the region lands in place.  Enqueued, not synchronised."""
        reg, w, h = _region(width, height, region)
        pitch, offset = (w if pitch is None else int(pitch)), int(offset)
        assert getattr(fb_tensor, "is_cuda", False), "fb: not a device tensor"
        assert fb_tensor.is_contiguous() and fb_tensor.element_size() == 4, "fb: want contiguous four-byte elements"
        assert pitch >= w and offset >= 0 and offset + (h - 1) * pitch + w <= fb_tensor.numel(), \
            f"fb: {h} rows of {w} elements at pitch {pitch} from element {offset} do not lie inside {fb_tensor.numel()} elements"
        _call("rrt_render_region_device", self._h, width, height, reg, _P(fb_tensor.data_ptr() + 4 * offset), pitch, _P(_stream(stream)))

    def render_tile_list_into(self, fb_tensor, tiles_t, width: int, height: int, stream: Optional[int] = None, bound_t=None):
        """rrt_render_tile_list_device: fb_tensor = a whole frame, width*height four-byte elements; tiles_t = a contiguous device tensor of four-byte tile indices
        ty * ((width + 7) // 8) + tx, in the order they are to be rendered (an index that names no tile is skipped); bound_t = None or a device tensor of one
        four-byte element: only the first min(len, bound) entries are read, by the kernel when it runs.  Enqueued, not synchronised."""
        _device_tensor(fb_tensor, width * height, 4, "fb")
        n = _batch_size(tiles_t, 1, "tiles")
        _device_tensor(tiles_t, n, 4, "tiles")
        if bound_t is not None:
            _device_tensor(bound_t, 1, 4, "bound")
        _call("rrt_render_tile_list_device", self._h, width, height, n, _ptr(bound_t), _ptr(tiles_t), _ptr(fb_tensor), _P(_stream(stream)))

    # tile selection (rrt.h: rrt_mark_tiles, rrt_select_tiles): tests over planes that produce the list render_tile_list_into reads
    def mark_tiles(self, test: CTileTest, width: int, height: int, region=None, marks=None) -> np.ndarray:
        """rrt_mark_tiles: [tiles_y][tiles_x] uint8, 1 where a pixel of the tile inside the region passes `test` (tile_test over host arrays).  marks: a
        contiguous uint8 array of that shape to write into (a test with keep joins what it holds); None: a new array of zeros."""
        reg, w, h = _region(width, height, region)
        tests, _ = _tile_tests("mark_tiles", test, w, h, False)
        tx, ty = tile_count(width, height)
        if marks is None:
            marks = np.zeros((ty, tx), np.uint8)
        assert isinstance(marks, np.ndarray) and marks.dtype == np.uint8 and marks.flags.c_contiguous and marks.flags.writeable and marks.size == tx * ty, \
            f"mark_tiles: marks is not a contiguous writable uint8 array of {tx * ty} elements"
        _call("rrt_mark_tiles", self._h, width, height, reg, tests, _u8(marks))
        return marks

    def select_tiles(self, tests, width: int, height: int, region=None) -> np.ndarray:
        """rrt_select_tiles: the ascending numbers ty * tiles_x + tx (uint32) of the tiles that some test of `tests` (1 to MAX_TILE_TESTS tile_test structs over
        host arrays) selects: their union."""
        reg, w, h = _region(width, height, region)
        arr, n = _tile_tests("select_tiles", tests, w, h, False)
        tx, ty = tile_count(width, height)
        tiles, count = np.empty(tx * ty, np.uint32), C.c_uint32(0)
        _call("rrt_select_tiles", self._h, width, height, reg, arr, n, _u32(tiles), C.byref(count))
        return tiles[:count.value].copy()

    def mark_tiles_into(self, marks_t, test: CTileTest, width: int, height: int, region=None, stream: Optional[int] = None):
        """rrt_mark_tiles_device: marks_t = tiles_x * tiles_y one-byte elements on the device; test = tile_test over device tensors.  Enqueued, not synchronised;
        last_stats stays as it was."""
        reg, w, h = _region(width, height, region)
        tests, _ = _tile_tests("mark_tiles_into", test, w, h, True)
        tx, ty = tile_count(width, height)
        _device_tensor(marks_t, tx * ty, 1, "marks")
        _call("rrt_mark_tiles_device", self._h, width, height, reg, tests, _ptr(marks_t), _P(_stream(stream)))

    def select_tiles_into(self, tiles_t, count_t, marks_t, scratch_t, tests, width: int, height: int, region=None, stream: Optional[int] = None):
        """rrt_select_tiles_device: tests = 1 to MAX_TILE_TESTS tile_test structs over device tensors; marks_t = n_tiles = tiles_x * tiles_y one-byte elements;
        tiles_t = n_tiles four-byte elements or None, count_t = one four-byte element or None (not both None); scratch_t = a device tensor of at least
        compact_scratch_bytes(n_tiles) bytes.  tiles_t and count_t are what render_tile_list_into takes as tiles_t and bound_t, on the same stream with nothing in
        between.  Enqueued, not synchronised; last_stats stays as it was."""
        reg, w, h = _region(width, height, region)
        arr, n = _tile_tests("select_tiles_into", tests, w, h, True)
        tx, ty = tile_count(width, height)
        _device_tensor(marks_t, tx * ty, 1, "marks")
        if tiles_t is not None:
            _device_tensor(tiles_t, tx * ty, 4, "tiles")
        if count_t is not None:
            _device_tensor(count_t, 1, 4, "count")
        assert tiles_t is not None or count_t is not None, "select_tiles_into: tiles and count are both None"
        assert getattr(scratch_t, "is_cuda", False) and scratch_t.is_contiguous(), "scratch: not a contiguous device tensor"
        _call("rrt_select_tiles_device", self._h, width, height, reg, arr, n, _ptr(marks_t), _ptr(tiles_t), _ptr(count_t), _ptr(scratch_t),
              scratch_t.numel() * scratch_t.element_size(), _P(_stream(stream)))

    # visibility buffers (rrt.h: rrt_render_visibility): first-hit geometry of the frame's primary rays.  region = (x0, y0, w, h) in canvas pixels, None = the frame
    def visibility(self, width: int, height: int, region=None, planes=PLANES) -> dict:
        """rrt_render_visibility: {plane: array [h][w][4]} of the region (last index: the sub-sample), only the planes asked for.  hit uint8, t / u / v
        float64, tri uint32 (push order, 0xFFFFFFFF = miss), albedo uint32 0x00RRGGBB."""
        reg, w, h = _region(width, height, region)
        out = _alloc_planes(CVisibility, planes, w, h)
        _call("rrt_render_visibility", self._h, width, height, reg, _plane_struct(CVisibility, out))
        return out

    def visibility_into(self, tensors: dict, width: int, height: int, region=None, stream: Optional[int] = None):
        """rrt_render_visibility_device: tensors = {plane: contiguous device tensor of 4*w*h elements of the plane's size}; enqueued, not synchronised."""
        reg, w, h = _region(width, height, region)
        _call("rrt_render_visibility_device", self._h, width, height, reg, _plane_struct(CVisibility, _device_planes(tensors, tensors, w, h)), _P(_stream(stream)))

    def pick(self, width: int, height: int, px: int, py: int) -> dict:
        """rrt_pick: what sub-sample 0 of canvas pixel (px, py) sees: dict hit (bool), tri, t, u, v, albedo."""
        r = CPickResult()
        _call("rrt_pick", self._h, width, height, px, py, C.byref(r))
        return dict(hit=bool(r.hit), tri=r.tri, t=r.t, u=r.u, v=r.v, albedo=r.albedo)

    # surface buffers (rrt.h: rrt_render_surface): hit point, shading normal, material index and light mask of the frame's primary rays
    def surface(self, width: int, height: int, region=None, planes=SURFACE_PLANES, visibility=()) -> dict:
        """rrt_render_surface: {plane: array} of the region, only the planes asked for.  point / normal float64 [h][w][4][3], material / lights uint32
        [h][w][4] (material 0xFFFFFFFF = miss; lights: bit k = light k reaches the point), and the visibility planes named in `visibility` ([h][w][4], as
        visibility() returns them) from the same launch."""
        reg, w, h = _region(width, height, region)
        out, vis = _alloc_planes(CSurface, planes, w, h), _alloc_planes(CVisibility, visibility, w, h)
        _call("rrt_render_surface", self._h, width, height, reg, _plane_struct(CVisibility, vis) if vis else None, _plane_struct(CSurface, out))
        out.update(vis)
        return out

    def surface_into(self, tensors: dict, width: int, height: int, region=None, stream: Optional[int] = None):
        """rrt_render_surface_device: tensors = {plane: contiguous device tensor}, keys from SURFACE_PLANES (12*w*h float64 for point / normal, 4*w*h four-byte
        elements for material / lights) and from PLANES (4*w*h elements of the plane's size); enqueued, not synchronised."""
        reg, w, h = _region(width, height, region)
        keep = _device_planes(tensors, tensors, w, h)
        _call("rrt_render_surface_device", self._h, width, height, reg, _plane_struct(CVisibility, keep), _plane_struct(CSurface, keep), _P(_stream(stream)))

    # shading from kept buffers (rrt.h: rrt_shade_surface): the frame of the planes surface() returned, with the lights and materials in force now
    def shade(self, width: int, height: int, planes: dict, region=None) -> np.ndarray:
        """rrt_shade_surface: planes = dict with point, normal ([h][w][4][3] float64), material, albedo ([h][w][4] uint32) and optionally lights, as
        surface(..., visibility=("albedo",)) returns them for this size and region; returns the region's pixels, [h][w] uint32 0x00RRGGBB.  Without `lights`
        the depth-0 shadow rays are walked again.  Other keys are ignored; a missing required plane is passed as NULL (the library refuses it)."""
        reg, w, h = _region(width, height, region)
        keep = _host_planes("shade", planes, SHADE_INPUTS, w, h)
        fb = np.empty((h, w), np.uint32)
        _call("rrt_shade_surface", self._h, width, height, reg, _plane_struct(CVisibility, keep), _plane_struct(CSurface, keep), _u32(fb))
        return fb

    def shade_into(self, fb_tensor, tensors: dict, width: int, height: int, region=None, stream: Optional[int] = None):
        """rrt_shade_surface_device: tensors = {plane: contiguous device tensor} with point, normal, material, albedo and optionally lights, as surface_into
        filled them; fb_tensor = w*h four-byte elements of the region; enqueued, not synchronised."""
        reg, w, h = _region(width, height, region)
        _device_tensor(fb_tensor, w * h, 4, "fb")
        keep = _device_planes(tensors, SHADE_INPUTS, w, h)
        _call("rrt_shade_surface_device", self._h, width, height, reg, _plane_struct(CVisibility, keep), _plane_struct(CSurface, keep), _ptr(fb_tensor),
              _P(_stream(stream)))

    # ambient occlusion from kept buffers (rrt.h: rrt_ambient_surface): which of the hemisphere rays `dirs` from every first hit are blocked
    def ambient(self, width: int, height: int, planes: dict, dirs, max_t: float = float("inf"), region=None, outputs=AMBIENT_OUTPUTS) -> dict:
        """rrt_ambient_surface: planes = dict with point, normal ([h][w][4][3] float64) and material ([h][w][4] uint32) as surface() returns them for this size
        and region (other keys are ignored; a missing plane is passed as NULL, which the library refuses); dirs = [n][3] directions in the tangent frame of a
        hit (z along the normal), n <= MAX_AMBIENT_SAMPLES; max_t as occluded() takes it.  Returns {"occluded": [h][w][4] uint32, bit k = ray k is blocked,
        "grey": [h][w] uint32 0x00GGGGGG, the share of open rays}, only the outputs asked for."""
        reg, w, h = _region(width, height, region)
        keep = _host_planes("ambient", planes, AMBIENT_INPUTS, w, h)
        _d_keep, samples = _ambient_samples(dirs, max_t)
        out = _alloc_planes(CAmbient, outputs, w, h)
        _call("rrt_ambient_surface", self._h, width, height, reg, _plane_struct(CSurface, keep), C.byref(samples), _plane_struct(CAmbient, out))
        return out

    def ambient_into(self, out_tensors: dict, plane_tensors: dict, dirs, max_t: float, width: int, height: int, region=None, stream: Optional[int] = None):
        """rrt_ambient_surface_device: plane_tensors = {plane: contiguous device tensor} with point, normal and material as surface_into filled them;
        out_tensors = {"occluded": 4*w*h four-byte elements, "grey": w*h four-byte elements} of the region, either or both; dirs (host, [n][3]) and max_t as
        ambient(); enqueued, not synchronised."""
        reg, w, h = _region(width, height, region)
        assert set(out_tensors) <= set(AMBIENT_OUTPUTS), sorted(out_tensors)
        out, keep = _device_planes(out_tensors, AMBIENT_OUTPUTS, w, h), _device_planes(plane_tensors, AMBIENT_INPUTS, w, h)
        _d_keep, samples = _ambient_samples(dirs, max_t)
        _call("rrt_ambient_surface_device", self._h, width, height, reg, _plane_struct(CSurface, keep), C.byref(samples), _plane_struct(CAmbient, out),
              _P(_stream(stream)))

    # the deferred stages over a device-resident tile list (rrt.h: rrt_render_visibility_tile_list_device and its three neighbours): every plane is a whole
    # frame, as the *_into twin takes it with region=None; tiles_t and bound_t as render_tile_list_into takes them (select_tiles_into writes both)
    def visibility_tile_list_into(self, tensors: dict, tiles_t, width: int, height: int, stream: Optional[int] = None, bound_t=None):
        """rrt_render_visibility_tile_list_device: tensors as visibility_into takes them for the whole frame; only the listed tiles' pixels are written.
        Enqueued, not synchronised."""
        keep = _device_planes(tensors, tensors, width, height)
        _call("rrt_render_visibility_tile_list_device", self._h, width, height, *_tile_list(tiles_t, bound_t), _plane_struct(CVisibility, keep), _P(_stream(stream)))

    def surface_tile_list_into(self, tensors: dict, tiles_t, width: int, height: int, stream: Optional[int] = None, bound_t=None):
        """rrt_render_surface_tile_list_device: tensors as surface_into takes them for the whole frame; only the listed tiles' pixels are written.
        Enqueued, not synchronised."""
        keep = _device_planes(tensors, tensors, width, height)
        _call("rrt_render_surface_tile_list_device", self._h, width, height, *_tile_list(tiles_t, bound_t), _plane_struct(CVisibility, keep),
              _plane_struct(CSurface, keep), _P(_stream(stream)))

    def shade_tile_list_into(self, fb_tensor, tensors: dict, tiles_t, width: int, height: int, stream: Optional[int] = None, bound_t=None):
        """rrt_shade_surface_tile_list_device: fb_tensor and tensors as shade_into takes them for the whole frame; the planes are read and the pixels written in
        the listed tiles only.  Enqueued, not synchronised."""
        _device_tensor(fb_tensor, width * height, 4, "fb")
        keep = _device_planes(tensors, SHADE_INPUTS, width, height)
        _call("rrt_shade_surface_tile_list_device", self._h, width, height, *_tile_list(tiles_t, bound_t), _plane_struct(CVisibility, keep),
              _plane_struct(CSurface, keep), _ptr(fb_tensor), _P(_stream(stream)))

    def ambient_tile_list_into(self, out_tensors: dict, plane_tensors: dict, dirs, max_t: float, tiles_t, width: int, height: int, stream: Optional[int] = None,
                               bound_t=None):
        """rrt_ambient_surface_tile_list_device: out_tensors, plane_tensors, dirs and max_t as ambient_into takes them for the whole frame; the planes are read
        and the outputs written in the listed tiles only.  Enqueued, not synchronised."""
        assert set(out_tensors) <= set(AMBIENT_OUTPUTS), sorted(out_tensors)
        out, keep = _device_planes(out_tensors, AMBIENT_OUTPUTS, width, height), _device_planes(plane_tensors, AMBIENT_INPUTS, width, height)
        _d_keep, samples = _ambient_samples(dirs, max_t)
        _call("rrt_ambient_surface_tile_list_device", self._h, width, height, *_tile_list(tiles_t, bound_t), _plane_struct(CSurface, keep), C.byref(samples),
              _plane_struct(CAmbient, out), _P(_stream(stream)))

    def setup_times(self) -> dict:
        """Wall ms of the once-per-scene stages: read, parse, texture decode, octree (model) + index, upload (this raytracer)."""
        t = CSetupTimes()
        _call("rrt_get_setup_times", self.scene_data._h if self.scene_data is not None else None, self._h, C.byref(t))
        return _struct_dict(t)

    def last_stats(self) -> dict:
        s = CStats()
        _call("rrt_last_stats", self._h, C.byref(s))
        return _struct_dict(s)


MULTI_LOOPBACK = 1   # RRT_MULTI_LOOPBACK


class MultiGpu(_Handle):
    """The N GPUs of one node behind one handle (include/rrt.h, rrt_multi): the screen-tile partition, the RCCL gather to rank 0 and the de-tiling
    all happen inside the library.  MultiGpu(raytracers) = one process driving every GPU (rrt_multi_create); MultiGpu.dist(rt, rank, world, unique_id)
    = one process per GPU (rrt_dist_create; rank 0 makes the id with MultiGpu.unique_id() and the caller broadcasts it)."""
    _destroy = "rrt_multi_destroy"

    def __init__(self, raytracers: Sequence["RayTracer"], frames_in_flight: int = 1, loopback: bool = False, _handle=None):
        self._keep = list(raytracers)
        if _handle is not None:
            self._h = _handle
            return
        arr = (_P * len(self._keep))(*[rt._h for rt in self._keep])
        out = _P()
        _call("rrt_multi_create", arr, len(self._keep), frames_in_flight, MULTI_LOOPBACK if loopback else 0, C.byref(out))
        self._h = out

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        _call("rrt_dist_unique_id", buf)
        return buf.raw

    @staticmethod
    def dist(rt: "RayTracer", rank: int, world: int, unique_id: Optional[bytes], frames_in_flight: int = 1) -> "MultiGpu":
        out = _P()
        idbuf = C.create_string_buffer(unique_id, 128) if unique_id is not None else None
        _call("rrt_dist_create", rt._h, rank, world, idbuf, frames_in_flight, C.byref(out))
        return MultiGpu([rt], _handle=out)

    def render(self, width: int, height: int) -> np.ndarray:
        """Blocking Scene::draw_scene over all GPUs, host framebuffer (rrt_render_multi)."""
        fb = np.empty((height, width), np.uint32)
        _call("rrt_render_multi", self._h, width, height, _u32(fb))
        return fb

    def bind_enqueue(self, fb_tensor, width: int, height: int):
        """One ctypes call per frame: trace -> gather -> de-tile enqueued on the next slot (fb_tensor on rank 0's GPU, None elsewhere)."""
        return _bound("rrt_multi_enqueue", self._h, C.c_uint32(width), C.c_uint32(height), _ptr(fb_tensor))

    def sync(self) -> None:
        _call("rrt_multi_sync", self._h)

    def last_gather_ms(self) -> float:
        v = C.c_double(-1.0)
        _call("rrt_multi_last_gather_ms", self._h, C.byref(v))
        return v.value


# ---------------------------------------------------------------------------------------------- host mirrors of the tile partition
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


# ---------------------------------------------------------------------------------------------- the reference's canvas and scene
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
