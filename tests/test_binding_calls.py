"""What the Python binding hands to the library, call by call, without a GPU and without the library: `rrt.lib` is replaced by a stand-in that records
(entry point, arguments) and answers with a programmable status; for getters a programmable reply writes through the out-pointers.  Arguments are recorded
in a neutral form -- ctypes scalars as values, byref(x) as x, structs as field dicts, arrays as lists, pointers as addresses -- so the records do not depend
on how the binding builds them.  The expected records below are written out from the contract in include/rrt.h; addresses are those of the arrays and
tensors the test passed in or of the arrays the method returned.

Device tensors are CPU torch tensors with is_cuda forced (data_ptr is a real host address); raytracers are made with RayTracer.__new__ and a made-up
handle, which is taken away again before the object dies so that nothing is ever freed.

Not here: the accepting path of tune_rays synchronises the current torch stream and therefore needs a GPU (tests/test_gpu_ray_queries.py); what it refuses
without one is in tests/test_ray_queries_abi.py."""
import ctypes as C
from collections import namedtuple

import numpy as np
import pytest

from abi_checks import fake_device

RT, SCENE, MULTI, STREAM = 0x1000, 0x2000, 0x3000, 0x51          # made-up handles and a made-up stream
W, H = 8, 4
REGION = (2, 1, 3, 2)                                            # x0, y0, w, h


class _NonNull:
    """Matches any address but NULL: for arrays the binding makes and keeps to itself (their contents are read by a reply, while the call is made)."""
    def __eq__(self, other):
        return isinstance(other, int) and other != 0
    def __repr__(self):
        return "<non-NULL>"


ANY = _NonNull()


def norm(a):
    if a is None or isinstance(a, (int, float, bytes)):
        return a
    if type(a).__name__ == "CArgObject":                          # byref(x)
        return norm(a._obj)
    if isinstance(a, C.Structure):
        return {n: norm(getattr(a, n)) for n, _ in a._fields_}
    if isinstance(a, C.Array):
        return a.raw if a._type_ is C.c_char else [norm(x) for x in a]
    if isinstance(a, C._Pointer) or isinstance(a, C._CFuncPtr):
        return C.cast(a, C.c_void_p).value
    if isinstance(a, C._SimpleCData):
        return a.value
    raise TypeError(f"argument of a kind the library cannot take: {a!r}")


class Recorder:
    """Stands in for the loaded library.  status[name]: what the entry point returns (default 0 = RRT_OK); replies[name](*raw arguments): runs during
    the call, after the arguments were recorded."""
    def __init__(self, status=None, replies=None):
        self.calls, self.raw, self.status, self.replies = [], [], dict(status or {}), dict(replies or {})

    def __getattr__(self, name):
        if name == "rrt_last_error_detail":
            return lambda: b"the detail"
        if name == "rrt_strerror":
            return lambda status: b"invalid argument"
        if name.endswith("_destroy"):                             # (an object dying during a case: nothing to record, nothing to free)
            return lambda handle: None

        def entry(*args):
            self.raw.append((name, args))
            self.calls.append((name, tuple(norm(a) for a in args)))
            if name in self.replies:
                self.replies[name](*args)
            return self.status.get(name, 0)
        return entry


def addr(a):
    """Address of a numpy array, a fake device tensor or a ctypes object."""
    return a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr() if hasattr(a, "data_ptr") else C.addressof(a)


def V(x, y, z):
    return dict(x=float(x), y=float(y), z=float(z))


def struct(names, **given):
    """A struct of pointers as recorded: NULL (None) except the fields given."""
    assert set(given) <= set(names.split()), given
    return {n: given.get(n) for n in names.split()}


def vis(**given):
    return struct("hit t u v tri albedo", **given)


def surf(**given):
    return struct("point normal material lights", **given)


def amb(**given):
    return struct("occluded grey", **given)


def zeros(cls):
    return norm(cls())


class Env:
    """The inputs every case draws from (fresh per case) and what replies have seen."""
    def __init__(self, rrt, region):
        import torch
        self.rrt, self.torch, self.seen = rrt, torch, []
        self.region = region
        self.reg = None if region is None else dict(x0=region[0], y0=region[1], w=region[2], h=region[3])
        self.w, self.h = (W, H) if region is None else (region[2], region[3])
        self.rt = rrt.RayTracer.__new__(rrt.RayTracer)
        self.rt._h, self.rt.scene_data, self.rt.device, self.rt.origin = C.c_void_p(RT), None, 0, rrt.DEFAULT_ORIGIN
        self.scene = type("StubScene", (), {})()
        self.scene._h = C.c_void_p(SCENE)
        self.mg = rrt.MultiGpu([self.rt], _handle=C.c_void_p(MULTI))
        self.made = [self.rt, self.mg]
        self.lights = [rrt.Light.Ambient(0.5), rrt.Light.Point(0.4, rrt.Vector3d(-7.0, 1.0, -15.0))]
        self.material = dict(ka=(0.1, 0.2, 0.3), kd=(0.4, 0.5, 0.6), ks=(0.7, 0.8, 0.9), ns=10, kr=0.25, tex=0)          # no bump key
        self.texture = np.arange(18, dtype=np.uint8).reshape(2, 3, 3)                                                    # 2 rows x 3 columns
        self.pos, self.uv, self.nrm = (np.arange(18.0).reshape(2, 3, 3) + k for k in (0.0, 100.0, 200.0))
        self.mat = np.zeros(2, np.uint32)
        self.o, self.d, self.max_t = np.zeros((4, 3)), np.ones((4, 3)), np.array([1.0, 2.0, 3.0, 4.0])
        self.dirs = [[0.0, 0.0, 1.0], [0.6, 0.0, 0.8]]
        self.fb = np.zeros((H, W), np.uint32)
        px = self.w * self.h
        f8 = lambda n: self.dev(torch.zeros(n, dtype=torch.float64))
        i4 = lambda n: self.dev(torch.zeros(n, dtype=torch.int32))
        self.t = dict(o=f8(12), d=f8(12), max_t=f8(4), out=self.dev(torch.zeros(4, dtype=torch.uint8)), t=f8(4), tri=i4(4), colours=i4(4), albedo4=i4(4),
                      pos=f8(18), uv=f8(18), nrm=f8(18), mat=i4(2), fb=i4(W * H), tiles=i4(64), gathered=i4(128), region_fb=i4(px),
                      hit=self.dev(torch.zeros(4 * px, dtype=torch.uint8)), vt=f8(4 * px), point=f8(12 * px), normal=f8(12 * px), material=i4(4 * px),
                      lights=i4(4 * px), albedo=i4(4 * px), occluded=i4(4 * px), grey=i4(px))
        self.planes = dict(point=np.zeros((self.h, self.w, 4, 3)), normal=np.ones((self.h, self.w, 4, 3)), material=np.zeros((self.h, self.w, 4), np.uint32),
                           lights=np.ones((self.h, self.w, 4), np.uint32), albedo=np.zeros((self.h, self.w, 4), np.uint32), junk="ignored")

    def dev(self, t):
        return fake_device(t, self.torch.device("cuda", 0))

    def scene_data(self):
        self.made.append(self.rrt.SceneData(SCENE))
        return self.made[-1]

    def without(self, d, *names):
        return {k: v for k, v in d.items() if k not in names}

    def release(self, *objects):
        for o in tuple(self.made) + objects:
            if isinstance(o, (self.rrt.SceneData, self.rrt.RayTracer, self.rrt.MultiGpu)):
                o._h = None


LIGHTS = [dict(kind=0, _pad=0, intensity=0.5, v=V(0, 0, 0)), dict(kind=1, _pad=0, intensity=0.4, v=V(-7, 1, -15))]
NO_LIGHT = dict(kind=0, _pad=0, intensity=0.0, v=V(0, 0, 0))
MATERIAL = dict(ka=V(0.1, 0.2, 0.3), kd=V(0.4, 0.5, 0.6), ks=V(0.7, 0.8, 0.9), ns=10.0, kr=0.25, tex=0, bump=-1)
ROOT = [-20.0, 20.0, -20.0, 20.0, -20.0, 20.0]                   # utils.rs:145
OTHER_ROOT = [-1.0, 2.0, -3.0, 4.0, -5.0, 6.0]
INFO = dict(n_tris=2, n_tris_in_tree=2, n_nodes=3, max_depth=2, n_mats=1, n_tex=1, root_own_count=1, max_own_count=1)


def options(flags, surface_offset=0.002, depth=3, vp=(2.0, 3.0, 4.0)):
    return dict(surface_offset=surface_offset, max_reflection_depth=depth, flags=flags, vp_w=vp[0], vp_h=vp[1], vp_d=vp[2])


def out_value(i, value):
    """A reply that stores `value` through the out-pointer at argument i (if it is given)."""
    def reply(*a):
        if a[i] is not None:
            a[i]._obj.value = value
    return reply


def out_fields(i, **fields):
    def reply(*a):
        if a[i] is not None:
            for k, v in fields.items():
                setattr(a[i]._obj, k, v)
    return reply


def counted(first):
    """rrt_raytracer_get_lights / _get_materials: *n_out = 1 or 2, and `first` into the array when there is one."""
    def reply(h, arr, cap, n_out):
        n_out._obj.value = 2
        if arr is not None:
            arr[1] = first
    return reply


def see(e, what):
    return lambda *a: e.seen.append(what(*a))


Case = namedtuple("Case", "name call expect replies status check raises", defaults=(None, None, None, None))
# call(e) -> result; expect(e, result) -> the records, in order; replies(e) -> {entry point: reply}; status: {entry point: what it returns};
# check(e, result): what the method returned; raises: (exception, words of its text) -- the records are still compared


def creation_cases():
    mk = lambda e, **kw: e.rrt.RayTracer(e.scene, e.lights, e.rrt.Vector3d(1.0, 2.0, 3.0), device=0, surface_offset=0.002, max_reflection_depth=3,
                                         viewport=(2, 3, 4), **kw)
    for kw, flags in (({}, 0), (dict(no_cull=True), 1), (dict(host_setup=True), 16), (dict(chain_shortcut=False), 32), (dict(box_filter="lane"), 2),
                      (dict(box_filter="bundle"), 4), (dict(box_filter="ray"), 8), (dict(no_cull=True, box_filter="ray", host_setup=True, chain_shortcut=False), 57)):
        yield Case(f"RayTracer({kw})", lambda e, kw=kw: mk(e, **kw),
                   lambda e, r, flags=flags: [("rrt_raytracer_create", (SCENE, LIGHTS, 2, V(1, 2, 3), options(flags), 0, None))],
                   replies=lambda e: {"rrt_raytracer_create": out_value(6, RT)}, check=lambda e, r: r._h.value == RT and r.scene_data is e.scene and r.device == 0)
    yield Case("RayTracer(no lights, default options)", lambda e: e.rrt.RayTracer(e.scene, [], device=3),
               lambda e, r: [("rrt_raytracer_create", (SCENE, [NO_LIGHT], 0, V(0, 2, -10), options(0, 0.0001, 5, (1.0, 1.0, 1.0)), 3, None))])
    scene = lambda e: (2, addr(e.pos), addr(e.uv), addr(e.nrm), addr(e.mat), 1, [MATERIAL], 1, [dict(rgb=addr(e.texture), width=3, height=2)])
    yield Case("RayTracer.from_arrays", lambda e: e.rrt.RayTracer.from_arrays(e.pos, e.uv, e.nrm, e.mat, [e.material], [e.texture], e.lights, device=1, no_cull=True,
                                                                              box_filter="bundle"),
               lambda e, r: [("rrt_raytracer_create_from_arrays", scene(e) + (ROOT, LIGHTS, 2, V(0, 2, -10), options(5, 0.0001, 5, (1.0, 1.0, 1.0)), 1, None))],
               replies=lambda e: {"rrt_raytracer_create_from_arrays": out_value(15, RT)}, check=lambda e, r: r._h.value == RT and r.scene_data is None and r.device == 1)
    yield Case("SceneData.from_arrays", lambda e: e.rrt.SceneData.from_arrays(e.pos, e.uv, e.nrm, e.mat, [e.material], [e.texture], root=OTHER_ROOT),
               lambda e, r: [("rrt_model_from_arrays", scene(e) + (OTHER_ROOT, None))],
               replies=lambda e: {"rrt_model_from_arrays": out_value(10, SCENE)}, check=lambda e, r: r._h.value == SCENE)


def scene_data_cases():
    info = lambda e: {"rrt_model_get_info": out_fields(1, **INFO)}
    yield Case("SceneData.info", lambda e: e.scene_data().info, lambda e, r: [("rrt_model_get_info", (SCENE, zeros(e.rrt.CModelInfo)))], replies=info,
               check=lambda e, r: r == INFO)
    yield Case("SceneData.materials", lambda e: e.scene_data().materials(),
               lambda e, r: [("rrt_model_get_info", (SCENE, zeros(e.rrt.CModelInfo))), ("rrt_model_get_materials", (SCENE, [zeros(e.rrt.CMaterial)]))],
               replies=lambda e: dict(info(e), rrt_model_get_materials=lambda h, cm: cm.__setitem__(0, e.rrt.CMaterial(ns=3.0, tex=2, bump=-1))),
               check=lambda e, r: r == [dict(ka=(0, 0, 0), kd=(0, 0, 0), ks=(0, 0, 0), ns=3.0, kr=0.0, tex=2, bump=-1)])
    yield Case("SceneData.octree", lambda e: e.scene_data().octree(),
               lambda e, r: [("rrt_model_get_info", (SCENE, zeros(e.rrt.CModelInfo))),
                             ("rrt_model_get_octree", (SCENE,) + tuple(addr(r[k]) for k in ("aabb", "first_child", "tri_count", "own_off", "own_idx")))],
               replies=info, check=lambda e, r: octree_ok(r))


def octree_ok(o, with_info=False):
    shapes = dict(aabb=((3, 6), np.float64), first_child=((3,), np.uint32), tri_count=((3,), np.uint32), own_off=((4,), np.uint32), own_idx=((2,), np.uint32))
    return (all(o[k].shape == s and o[k].dtype == t for k, (s, t) in shapes.items()) and o["max_depth"] == 2
            and set(o) == set(shapes) | {"max_depth"} | ({"info"} if with_info else set()) and (not with_info or o["info"] == INFO))


def update_cases():
    yield Case("set_lights", lambda e: e.rt.set_lights(iter(e.lights)), lambda e, r: [("rrt_raytracer_set_lights", (RT, LIGHTS, 2))])
    yield Case("set_lights([])", lambda e: e.rt.set_lights([]), lambda e, r: [("rrt_raytracer_set_lights", (RT, [NO_LIGHT], 0))])
    yield Case("lights", lambda e: e.rt.lights(),
               lambda e, r: [("rrt_raytracer_get_lights", (RT, None, 0, 0)), ("rrt_raytracer_get_lights", (RT, [NO_LIGHT, NO_LIGHT], 2, 2))],
               replies=lambda e: {"rrt_raytracer_get_lights": counted(e.rrt.CLight(2, 0, 0.25, e.rrt.Vec3(1.0, 2.0, 3.0)))},
               check=lambda e, r: r == [e.rrt.Light(0, 0.0, e.rrt.Vector3d(0.0, 0.0, 0.0)), e.rrt.Light.Directional(0.25, e.rrt.Vector3d(1.0, 2.0, 3.0))])
    yield Case("set_materials", lambda e: e.rt.set_materials([e.material]), lambda e, r: [("rrt_raytracer_set_materials", (RT, [MATERIAL], 1))])
    yield Case("materials", lambda e: e.rt.materials(),
               lambda e, r: [("rrt_raytracer_get_materials", (RT, None, 0, 0)), ("rrt_raytracer_get_materials", (RT, [zeros(e.rrt.CMaterial)] * 2, 2, 2))],
               replies=lambda e: {"rrt_raytracer_get_materials": counted(e.rrt.CMaterial(kd=e.rrt.Vec3(1.0, 2.0, 3.0), ns=3.0, tex=2, bump=4))},
               check=lambda e, r: r == [dict(ka=(0, 0, 0), kd=(0, 0, 0), ks=(0, 0, 0), ns=0.0, kr=0.0, tex=0, bump=0),
                                        dict(ka=(0, 0, 0), kd=(1.0, 2.0, 3.0), ks=(0, 0, 0), ns=3.0, kr=0.0, tex=2, bump=4)])
    tris = lambda e: (RT, 2, addr(e.pos), addr(e.uv), addr(e.nrm), addr(e.mat))
    yield Case("set_triangles", lambda e: e.rt.set_triangles(e.pos, e.uv, e.nrm, e.mat), lambda e, r: [("rrt_raytracer_set_triangles", tris(e) + (None,))])
    yield Case("set_triangles(root)", lambda e: e.rt.set_triangles(e.pos, e.uv, e.nrm, e.mat, root=(-1, 2, -3, 4, -5, 6)),
               lambda e, r: [("rrt_raytracer_set_triangles", tris(e) + (OTHER_ROOT,))])
    for root in (None, OTHER_ROOT):
        yield Case(f"set_triangles: sizes disagree (root {root})", lambda e, root=root: e.rt.set_triangles(e.pos, e.uv, e.nrm, np.zeros(3, np.uint32), root=root),
                   lambda e, r: [], raises=(ValueError, "2 positions, 2 uv, 2 normals, 3 material indices"))
    dev = lambda e: (RT, 2, addr(e.t["pos"]), addr(e.t["uv"]), addr(e.t["nrm"]), addr(e.t["mat"]))
    yield Case("set_triangles_from", lambda e: e.rt.set_triangles_from(e.t["pos"], e.t["uv"], e.t["nrm"], e.t["mat"], stream=STREAM),
               lambda e, r: [("rrt_raytracer_set_triangles_device", dev(e) + (None, STREAM))])
    yield Case("set_triangles_from(root)", lambda e: e.rt.set_triangles_from(e.t["pos"], e.t["uv"], e.t["nrm"], e.t["mat"], root=OTHER_ROOT, stream=STREAM),
               lambda e, r: [("rrt_raytracer_set_triangles_device", dev(e) + (OTHER_ROOT, STREAM))])
    yield Case("set_triangles_from: host tensors", lambda e: e.rt.set_triangles_from(*(e.torch.zeros(18, dtype=e.torch.float64),) * 3, e.torch.zeros(2, dtype=e.torch.int32),
                                                                                     stream=STREAM),
               lambda e, r: [], raises=(ValueError, "set_triangles_from: pos: not a device tensor"))
    yield Case("set_triangles_from: three material indices", lambda e: e.rt.set_triangles_from(e.t["pos"], e.t["uv"], e.t["nrm"], e.dev(e.torch.zeros(3, dtype=e.torch.int32)),
                                                                                               stream=STREAM),
               lambda e, r: [], raises=(ValueError, "mat"))
    yield Case("release_update_memory", lambda e: e.rt.release_update_memory(), lambda e, r: [("rrt_raytracer_release_update_memory", (RT,))])


def ray_cases():
    doubles = lambda i: lambda *a: [a[i][k] for k in range(4)]                     # the four doubles behind argument i, read during the call
    yield Case("get_ray_colours", lambda e: e.rt.get_ray_colours(e.o, e.d), lambda e, r: [("rrt_get_ray_colours", (RT, 4, addr(e.o), addr(e.d), addr(r)))],
               check=lambda e, r: r.shape == (4,) and r.dtype == np.uint32)
    yield Case("get_ray_colour", lambda e: e.rt.get_ray_colour(e.rrt.Vector3d(1, 2, 3), e.rrt.Vector3d(4, 5, 6)),
               lambda e, r: [("rrt_get_ray_colours", (RT, 1, ANY, ANY, ANY))],
               replies=lambda e: {"rrt_get_ray_colours": lambda h, n, o, d, out: (e.seen.append([o[k] for k in range(3)] + [d[k] for k in range(3)]), out.__setitem__(0, 0x123456))},
               check=lambda e, r: r == 0x123456 and e.seen == [[1.0, 2.0, 3.0, 4.0, 5.0, 6.0]])
    ok5 = lambda e, r: (r[0].dtype == bool and [a.dtype for a in r[1:]] == [np.float64] * 3 + [np.uint32] and all(a.shape == (4,) for a in r))
    out5 = lambda r: (ANY, addr(r[1]), addr(r[2]), addr(r[3]), addr(r[4]))
    yield Case("intersect_rays", lambda e: e.rt.intersect_rays(e.o, e.d), lambda e, r: [("rrt_intersect_rays", (RT, 4, addr(e.o), addr(e.d), None) + out5(r))], check=ok5)
    yield Case("intersect_rays(max_t scalar)", lambda e: e.rt.intersect_rays(e.o, e.d, 2.5),
               lambda e, r: [("rrt_intersect_rays", (RT, 4, addr(e.o), addr(e.d), ANY) + out5(r))],
               replies=lambda e: {"rrt_intersect_rays": see(e, doubles(4))}, check=lambda e, r: ok5(e, r) and e.seen == [[2.5] * 4])
    yield Case("intersect_rays(max_t array)", lambda e: e.rt.intersect_rays(e.o, e.d, e.max_t),
               lambda e, r: [("rrt_intersect_rays", (RT, 4, addr(e.o), addr(e.d), addr(e.max_t)) + out5(r))], check=ok5)
    okb = lambda e, r: r.dtype == bool and r.shape == (4,)
    yield Case("occluded", lambda e: e.rt.occluded(e.o, e.d), lambda e, r: [("rrt_occluded_rays", (RT, 4, addr(e.o), addr(e.d), None, ANY))], check=okb)
    yield Case("occluded(max_t scalar)", lambda e: e.rt.occluded(e.o, e.d, 2.5), lambda e, r: [("rrt_occluded_rays", (RT, 4, addr(e.o), addr(e.d), ANY, ANY))],
               replies=lambda e: {"rrt_occluded_rays": lambda h, n, o, d, mt, out: (e.seen.append([mt[k] for k in range(4)]), [out.__setitem__(k, int(k == 2)) for k in range(4)])},
               check=lambda e, r: okb(e, r) and e.seen == [[2.5] * 4] and r.tolist() == [False, False, True, False])
    yield Case("occluded(max_t array)", lambda e: e.rt.occluded(e.o, e.d, e.max_t), lambda e, r: [("rrt_occluded_rays", (RT, 4, addr(e.o), addr(e.d), addr(e.max_t), ANY))],
               check=okb)
    rays = lambda e: (RT, 4, addr(e.t["o"]), addr(e.t["d"]))
    yield Case("occluded_into", lambda e: e.rt.occluded_into(e.t["o"], e.t["d"], e.t["out"], e.t["max_t"], stream=STREAM),
               lambda e, r: [("rrt_occluded_rays_device", rays(e) + (addr(e.t["max_t"]), addr(e.t["out"]), STREAM))])
    yield Case("occluded_into(no max_t)", lambda e: e.rt.occluded_into(e.t["o"], e.t["d"], e.t["out"], stream=STREAM),
               lambda e, r: [("rrt_occluded_rays_device", rays(e) + (None, addr(e.t["out"]), STREAM))])
    yield Case("intersect_rays_into({t, tri})", lambda e: e.rt.intersect_rays_into(e.t["o"], e.t["d"], {"tri": e.t["tri"], "t": e.t["t"]}, stream=STREAM),
               lambda e, r: [("rrt_intersect_rays_device", rays(e) + (None, None, addr(e.t["t"]), None, None, addr(e.t["tri"]), STREAM))])       # hit t u v tri
    yield Case("intersect_rays_into(max_t)", lambda e: e.rt.intersect_rays_into(e.t["o"], e.t["d"], {"hit": e.t["out"]}, e.t["max_t"], stream=STREAM),
               lambda e, r: [("rrt_intersect_rays_device", rays(e) + (addr(e.t["max_t"]), addr(e.t["out"]), None, None, None, None, STREAM))])
    yield Case("intersect_rays_into refuses albedo", lambda e: e.rt.intersect_rays_into(e.t["o"], e.t["d"], {"albedo": e.t["albedo4"]}, stream=STREAM),
               lambda e, r: [], raises=(AssertionError, "albedo"))
    yield Case("get_ray_colours_into", lambda e: e.rt.get_ray_colours_into(e.t["o"], e.t["d"], e.t["colours"], stream=STREAM),
               lambda e, r: [("rrt_get_ray_colours_device", rays(e) + (addr(e.t["colours"]), STREAM))])


def frame_cases():
    frame = lambda e, r: r.shape == (H, W) and r.dtype == np.uint32
    yield Case("render", lambda e: e.rt.render(W, H), lambda e, r: [("rrt_render", (RT, W, H, addr(r)))], check=frame)
    yield Case("render_into", lambda e: e.rt.render_into(e.t["fb"], W, H, stream=STREAM), lambda e, r: [("rrt_render_device", (RT, W, H, addr(e.t["fb"]), STREAM))])
    one_tile_each = {"rrt_tiles_per_rank": 1}                                       # an 8 x 4 frame is one 8 x 8 tile: ceil(1 / 2) per rank
    yield Case("render_tiles_into", lambda e: e.rt.render_tiles_into(e.t["tiles"], W, H, 1, 2, stream=STREAM),
               lambda e, r: [("rrt_tiles_per_rank", (W, H, 2)), ("rrt_render_tiles_device", (RT, W, H, 1, 2, addr(e.t["tiles"]), STREAM))], status=one_tile_each)
    yield Case("detile_into", lambda e: e.rt.detile_into(e.t["gathered"], e.t["fb"], W, H, 2, stream=STREAM),
               lambda e, r: [("rrt_tiles_per_rank", (W, H, 2)), ("rrt_detile_device", (RT, W, H, 2, addr(e.t["gathered"]), addr(e.t["fb"]), STREAM))],
               status=one_tile_each)
    update = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32)     # rrt_update_fn
    yield Case("render_progressive", lambda e: e.rt.render_progressive(W, H, lambda fb, row0, rows: e.seen.append((fb, row0, rows)), chunk_rows=2),
               lambda e, r: [("rrt_render_progressive", (RT, W, H, addr(r), 2, ANY, None))],
               replies=lambda e: {"rrt_render_progressive": lambda h, w, hh, fb, rows, cb, user: C.cast(cb, update)(user, C.cast(fb, C.c_void_p), w, hh, 2, 2)},
               check=lambda e, r: frame(e, r) and len(e.seen) == 1 and e.seen[0][0] is r and e.seen[0][1:] == (2, 2))
    yield Case("render_progressive(no callback)", lambda e: e.rt.render_progressive(W, H), lambda e, r: [("rrt_render_progressive", (RT, W, H, addr(r), 50, None, None))])
    registered = lambda e, r: [("rrt_host_buffer_register", (addr(e.fb), 128)), ("rrt_render", (RT, W, H, addr(e.fb))), ("rrt_host_buffer_unregister", (addr(e.fb),))]
    yield Case("render_registered", lambda e: e.rt.render_registered(W, H, e.fb), registered, check=lambda e, r: r is e.fb)
    yield Case("render_registered(own buffer)", lambda e: e.rt.render_registered(W, H),
               lambda e, r: [("rrt_host_buffer_register", (addr(r), 128)), ("rrt_render", (RT, W, H, addr(r))), ("rrt_host_buffer_unregister", (addr(r),))], check=frame)
    yield Case("render_registered: the render fails", lambda e: e.rt.render_registered(W, H, e.fb), registered, status={"rrt_render": -2},
               raises=("RrtError", "rrt_render failed"))
    yield Case("Scene.draw_scene", lambda e: (lambda s: (s.draw_scene(e.rt), s)[1])(e.rrt.Scene(W, H)),
               lambda e, r: [("rrt_render", (RT, W, H, addr(r.canvas.buffer)))], check=lambda e, r: r.canvas.updates == 1)


def region_cases(region):
    tag = "frame" if region is None else "region"
    yield Case(f"visibility, {tag}", lambda e: e.rt.visibility(W, H, region),
               lambda e, r: [("rrt_render_visibility", (RT, W, H, e.reg, vis(**{k: addr(a) for k, a in r.items()})))],
               check=lambda e, r: ({k: a.dtype for k, a in r.items()} == dict(hit=np.uint8, t=np.float64, u=np.float64, v=np.float64, tri=np.uint32, albedo=np.uint32)
                                   and all(a.shape == (e.h, e.w, 4) for a in r.values())))
    yield Case(f"visibility(t, tri), {tag}", lambda e: e.rt.visibility(W, H, region, planes=("tri", "t")),
               lambda e, r: [("rrt_render_visibility", (RT, W, H, e.reg, vis(t=addr(r["t"]), tri=addr(r["tri"]))))], check=lambda e, r: sorted(r) == ["t", "tri"])
    yield Case(f"visibility_into, {tag}", lambda e: e.rt.visibility_into({"t": e.t["vt"], "hit": e.t["hit"]}, W, H, region, stream=STREAM),
               lambda e, r: [("rrt_render_visibility_device", (RT, W, H, e.reg, vis(hit=addr(e.t["hit"]), t=addr(e.t["vt"])), STREAM))])
    yield Case(f"visibility_into: a plane of the frame's size for a region ({tag})" if region else f"visibility_into: float32 t ({tag})",
               lambda e: e.rt.visibility_into({"t": e.dev(e.torch.zeros(4 * W * H, dtype=e.torch.float64 if region else e.torch.float32))}, W, H, region, stream=STREAM),
               lambda e, r: [], raises=(AssertionError, "t"))
    surface_shapes = lambda e, r: ({k: (a.dtype, a.shape) for k, a in r.items() if k in e.rrt.SURFACE_PLANES}
                                   == dict(point=(np.float64, (e.h, e.w, 4, 3)), normal=(np.float64, (e.h, e.w, 4, 3)), material=(np.uint32, (e.h, e.w, 4)),
                                           lights=(np.uint32, (e.h, e.w, 4))))
    yield Case(f"surface, {tag}", lambda e: e.rt.surface(W, H, region),
               lambda e, r: [("rrt_render_surface", (RT, W, H, e.reg, None, surf(**{k: addr(a) for k, a in r.items()})))],              # no visibility plane: NULL, not a struct
               check=lambda e, r: surface_shapes(e, r) and len(r) == 4)
    yield Case(f"surface(point + albedo, hit), {tag}", lambda e: e.rt.surface(W, H, region, planes=("point",), visibility=("albedo", "hit")),
               lambda e, r: [("rrt_render_surface", (RT, W, H, e.reg, vis(albedo=addr(r["albedo"]), hit=addr(r["hit"])), surf(point=addr(r["point"]))))],
               check=lambda e, r: (sorted(r) == ["albedo", "hit", "point"] and r["albedo"].shape == r["hit"].shape == (e.h, e.w, 4)
                                   and (r["albedo"].dtype, r["hit"].dtype) == (np.uint32, np.uint8)))
    yield Case(f"surface_into, {tag}", lambda e: e.rt.surface_into({k: e.t[k] for k in ("point", "normal", "material", "lights")}, W, H, region, stream=STREAM),
               lambda e, r: [("rrt_render_surface_device", (RT, W, H, e.reg, vis(), surf(**{k: addr(e.t[k]) for k in ("point", "normal", "material", "lights")}), STREAM))])
    yield Case(f"surface_into(lights + albedo), {tag}", lambda e: e.rt.surface_into({"albedo": e.t["albedo"], "lights": e.t["lights"]}, W, H, region, stream=STREAM),
               lambda e, r: [("rrt_render_surface_device", (RT, W, H, e.reg, vis(albedo=addr(e.t["albedo"])), surf(lights=addr(e.t["lights"])), STREAM))])
    yield Case(f"surface_into: four-byte point, {tag}", lambda e: e.rt.surface_into({"point": e.dev(e.torch.zeros(12 * e.w * e.h))}, W, H, region, stream=STREAM),
               lambda e, r: [], raises=(AssertionError, "point"))
    kept = lambda e, *names: {k: addr(e.planes[k]) for k in names}
    yield Case(f"shade, {tag}", lambda e: e.rt.shade(W, H, e.planes, region),
               lambda e, r: [("rrt_shade_surface", (RT, W, H, e.reg, vis(**kept(e, "albedo")), surf(**kept(e, "point", "normal", "material", "lights")), addr(r)))],
               check=lambda e, r: r.shape == (e.h, e.w) and r.dtype == np.uint32)
    yield Case(f"shade without lights and normal, {tag}", lambda e: e.rt.shade(W, H, e.without(e.planes, "lights", "normal"), region),
               lambda e, r: [("rrt_shade_surface", (RT, W, H, e.reg, vis(**kept(e, "albedo")), surf(**kept(e, "point", "material")), addr(r)))])   # NULL, no exception
    yield Case(f"shade without any plane, {tag}", lambda e: e.rt.shade(W, H, {}, region), lambda e, r: [("rrt_shade_surface", (RT, W, H, e.reg, vis(), surf(), addr(r)))])
    yield Case(f"shade: a plane of another size, {tag}", lambda e: e.rt.shade(W, H, dict(e.planes, material=np.zeros((e.h, e.w + 1, 4), np.uint32)), region),
               lambda e, r: [], raises=(ValueError, f"material has shape ({e_h(region)}, {e_w(region) + 1}, 4), want ({e_h(region)}, {e_w(region)}, 4)"))
    dkept = lambda e, *names: {k: addr(e.t[k]) for k in names}
    device_planes = lambda e: {k: e.t[k] for k in ("point", "normal", "material", "lights", "albedo")}
    yield Case(f"shade_into, {tag}", lambda e: e.rt.shade_into(e.t["region_fb"], dict(device_planes(e), junk=None), W, H, region, stream=STREAM),
               lambda e, r: [("rrt_shade_surface_device", (RT, W, H, e.reg, vis(**dkept(e, "albedo")), surf(**dkept(e, "point", "normal", "material", "lights")),
                                                           addr(e.t["region_fb"]), STREAM))])
    yield Case(f"shade_into without any plane, {tag}", lambda e: e.rt.shade_into(e.t["region_fb"], {}, W, H, region, stream=STREAM),
               lambda e, r: [("rrt_shade_surface_device", (RT, W, H, e.reg, vis(), surf(), addr(e.t["region_fb"]), STREAM))])
    yield Case(f"shade_into: a framebuffer of sub-samples, {tag}", lambda e: e.rt.shade_into(e.t["albedo"], device_planes(e), W, H, region, stream=STREAM),
               lambda e, r: [], raises=(AssertionError, "fb"))
    samples = lambda max_t: dict(dirs=ANY, n=2, _pad=0, max_t=max_t)
    six = lambda i: lambda *a: [a[i]._obj.dirs[k] for k in range(6)]               # the direction doubles, read during the call
    dirs_seen = lambda e: e.seen == [[0.0, 0.0, 1.0, 0.6, 0.0, 0.8]]
    yield Case(f"ambient, {tag}", lambda e: e.rt.ambient(W, H, e.planes, e.dirs, 2.5, region),
               lambda e, r: [("rrt_ambient_surface", (RT, W, H, e.reg, surf(**kept(e, "point", "normal", "material")), samples(2.5),
                                                      amb(occluded=addr(r["occluded"]), grey=addr(r["grey"]))))],
               replies=lambda e: {"rrt_ambient_surface": see(e, six(5))},
               check=lambda e, r: (dirs_seen(e) and r["occluded"].shape == (e.h, e.w, 4) and r["grey"].shape == (e.h, e.w)
                                   and r["occluded"].dtype == r["grey"].dtype == np.uint32))
    yield Case(f"ambient(grey, no max_t, no material), {tag}", lambda e: e.rt.ambient(W, H, e.without(e.planes, "material"), np.array(e.dirs), region=region, outputs=("grey",)),
               lambda e, r: [("rrt_ambient_surface", (RT, W, H, e.reg, surf(**kept(e, "point", "normal")), samples(float("inf")), amb(grey=addr(r["grey"]))))],
               check=lambda e, r: list(r) == ["grey"])
    yield Case(f"ambient: a plane of another size, {tag}", lambda e: e.rt.ambient(W, H, dict(e.planes, point=np.zeros((e.h, e.w, 4))), e.dirs, region=region),
               lambda e, r: [], raises=(ValueError, f"point has shape ({e_h(region)}, {e_w(region)}, 4), want ({e_h(region)}, {e_w(region)}, 4, 3)"))
    yield Case(f"ambient_into, {tag}", lambda e: e.rt.ambient_into({"occluded": e.t["occluded"], "grey": e.t["grey"]}, device_planes(e), e.dirs, 2.5, W, H, region, stream=STREAM),
               lambda e, r: [("rrt_ambient_surface_device", (RT, W, H, e.reg, surf(**dkept(e, "point", "normal", "material")), samples(2.5),
                                                             amb(occluded=addr(e.t["occluded"]), grey=addr(e.t["grey"])), STREAM))],
               replies=lambda e: {"rrt_ambient_surface_device": see(e, six(5))}, check=lambda e, r: dirs_seen(e))
    yield Case(f"ambient_into(occluded, no normal), {tag}", lambda e: e.rt.ambient_into({"occluded": e.t["occluded"]}, {"point": e.t["point"], "material": e.t["material"]},
                                                                                        e.dirs, float("inf"), W, H, region, stream=STREAM),
               lambda e, r: [("rrt_ambient_surface_device", (RT, W, H, e.reg, surf(**dkept(e, "point", "material")), samples(float("inf")),
                                                             amb(occluded=addr(e.t["occluded"])), STREAM))])
    yield Case(f"ambient_into: grey of sub-samples, {tag}", lambda e: e.rt.ambient_into({"grey": e.t["occluded"]}, device_planes(e), e.dirs, 2.5, W, H, region, stream=STREAM),
               lambda e, r: [], raises=(AssertionError, "grey"))


def e_w(region):
    return W if region is None else region[2]


def e_h(region):
    return H if region is None else region[3]


def query_cases():
    yield Case("pick", lambda e: e.rt.pick(W, H, 5, 2), lambda e, r: [("rrt_pick", (RT, W, H, 5, 2, zeros(e.rrt.CPickResult)))],
               replies=lambda e: {"rrt_pick": out_fields(5, hit=1, tri=7, t=1.5, u=0.25, v=0.5, albedo=0x102030)},
               check=lambda e, r: r == dict(hit=True, tri=7, t=1.5, u=0.25, v=0.5, albedo=0x102030) and r["hit"] is True)
    pose = dict(eye=V(1, 2, 3), right=V(0, 0, 1), up=V(0, 1, 0), forward=V(-1, 0, 0))
    yield Case("set_camera", lambda e: e.rt.set_camera((1, 2, 3), right=(0, 0, 1), forward=e.rrt.Vector3d(-1, 0, 0)), lambda e, r: [("rrt_raytracer_set_camera", (RT, pose))])
    yield Case("set_camera(eye)", lambda e: e.rt.set_camera((1, 2, 3)),
               lambda e, r: [("rrt_raytracer_set_camera", (RT, dict(eye=V(1, 2, 3), right=V(1, 0, 0), up=V(0, 1, 0), forward=V(0, 0, 1))))])
    yield Case("reset_camera", lambda e: e.rt.reset_camera(), lambda e, r: [("rrt_raytracer_set_camera", (RT, None))])
    fill_pose = lambda e, i: out_fields(i, eye=e.rrt.Vec3(1, 2, 3), right=e.rrt.Vec3(0, 0, 1), up=e.rrt.Vec3(0, 1, 0), forward=e.rrt.Vec3(-1, 0, 0))
    as_tuples = dict(eye=(1.0, 2.0, 3.0), right=(0.0, 0.0, 1.0), up=(0.0, 1.0, 0.0), forward=(-1.0, 0.0, 0.0))
    yield Case("camera", lambda e: e.rt.camera(), lambda e, r: [("rrt_raytracer_get_camera", (RT, zeros(e.rrt.CCamera)))],
               replies=lambda e: {"rrt_raytracer_get_camera": fill_pose(e, 1)}, check=lambda e, r: r == as_tuples)
    yield Case("look_at (module)", lambda e: e.rrt.look_at((1, 2, 3), e.rrt.Vector3d(0, 2, 3)),
               lambda e, r: [("rrt_camera_look_at", (V(1, 2, 3), V(0, 2, 3), V(0, 1, 0), zeros(e.rrt.CCamera)))],
               replies=lambda e: {"rrt_camera_look_at": fill_pose(e, 3)}, check=lambda e, r: r == as_tuples)
    yield Case("look_at (method)", lambda e: e.rt.look_at((1, 2, 3), (0, 2, 3), up=(0, 0, 1)),
               lambda e, r: [("rrt_camera_look_at", (V(1, 2, 3), V(0, 2, 3), V(0, 0, 1), zeros(e.rrt.CCamera))), ("rrt_raytracer_set_camera", (RT, pose))],
               replies=lambda e: {"rrt_camera_look_at": fill_pose(e, 3)})
    info_only = lambda e: (RT, zeros(e.rrt.CModelInfo), None, None, None, None, None)
    fill_info = lambda e: {"rrt_raytracer_get_octree": out_fields(1, **INFO)}
    yield Case("info", lambda e: e.rt.info, lambda e, r: [("rrt_raytracer_get_octree", info_only(e))], replies=fill_info, check=lambda e, r: r == INFO)
    yield Case("octree", lambda e: e.rt.octree(),
               lambda e, r: [("rrt_raytracer_get_octree", info_only(e)),
                             ("rrt_raytracer_get_octree", (RT, None) + tuple(addr(r[k]) for k in ("aabb", "first_child", "tri_count", "own_off", "own_idx")))],
               replies=fill_info, check=lambda e, r: octree_ok(r, with_info=True))
    yield Case("chain_info", lambda e: e.rt.chain_info, lambda e, r: [("rrt_raytracer_get_chain_info", (RT, 0, 0))],
               replies=lambda e: {"rrt_raytracer_get_chain_info": lambda h, a, b: (setattr(a._obj, "value", 3), setattr(b._obj, "value", 9))},
               check=lambda e, r: r == {"n_chains": 3, "n_chain_nodes": 9})
    fill_cover = lambda state, waves, empty: lambda h, s_, w_, e_: (setattr(s_._obj, "value", state), setattr(w_._obj, "value", waves),
                                                                      e_ is not None and setattr(e_._obj, "value", empty))
    yield Case("coverage_info", lambda e: e.rt.coverage_info(), lambda e, r: [("rrt_raytracer_get_coverage_info", (RT, 0, 0, None))],
               replies=lambda e: {"rrt_raytracer_get_coverage_info": fill_cover(9, 0, 0)}, check=lambda e, r: r == {"state": "small_frame", "n_waves": 0})
    yield Case("coverage_info(count)", lambda e: e.rt.coverage_info(count=True), lambda e, r: [("rrt_raytracer_get_coverage_info", (RT, 0, 0, 0))],
               replies=lambda e: {"rrt_raytracer_get_coverage_info": fill_cover(0, 48, 7)}, check=lambda e, r: r == {"state": "on", "n_waves": 48, "n_proved_empty": 7})
    # coverage_mask: a 20 x 12 frame has 3 x 2 tiles = 24 waves in ONE word; the reply sets the bits of waves (bx 5, by 0) and (bx 2, by 3):
    # ((0 * 3 + 2) * 4 | 0 | 1) = 9 and ((1 * 3 + 1) * 4 | 2 | 0) = 18
    def mask_reply(h, words, n):
        words[0] = (1 << 9) | (1 << 18)
    mask_want = np.zeros((4, 6), bool); mask_want[0, 5] = mask_want[3, 2] = True
    yield Case("coverage_mask", lambda e: e.rt.coverage_mask(),
               lambda e, r: [("rrt_raytracer_get_coverage_info", (RT, 0, 0, None)), ("rrt_last_stats", (RT, zeros(e.rrt.CStats))), ("rrt_raytracer_get_coverage_mask", (RT, ANY, 1))],
               replies=lambda e: {"rrt_raytracer_get_coverage_info": fill_cover(0, 24, 0), "rrt_last_stats": out_fields(1, width=20, height=12),
                                  "rrt_raytracer_get_coverage_mask": mask_reply},
               check=lambda e, r: r.dtype == bool and r.shape == (4, 6) and np.array_equal(r, mask_want))
    yield Case("coverage_mask(no mask)", lambda e: e.rt.coverage_mask(), lambda e, r: [("rrt_raytracer_get_coverage_info", (RT, 0, 0, None))],
               replies=lambda e: {"rrt_raytracer_get_coverage_info": fill_cover(5, 0, 0)}, check=lambda e, r: r is None)
    yield Case("buffer", lambda e: e.rt.buffer("attr"),                                                              # RRT_BUF_ATTR = 2
               lambda e, r: [("rrt_raytracer_get_buffer", (RT, 2, None, 0, 0)), ("rrt_raytracer_get_buffer", (RT, 2, addr(r), 5, None))],
               replies=lambda e: {"rrt_raytracer_get_buffer": out_value(4, 5)}, check=lambda e, r: r.shape == (5,) and r.dtype == np.uint8)
    times = dict(read_ms=1.0, parse_ms=2.0, texture_ms=3.0, octree_ms=4.0, index_ms=5.0, upload_ms=6.0, hip_init_ms=7.0, create_ms=8.0, gpu_setup=1.0)
    yield Case("setup_times", lambda e: e.rt.setup_times(), lambda e, r: [("rrt_get_setup_times", (None, RT, zeros(e.rrt.CSetupTimes)))],
               replies=lambda e: {"rrt_get_setup_times": out_fields(2, **times)}, check=lambda e, r: r == times)
    yield Case("setup_times(with a model)", lambda e: (setattr(e.rt, "scene_data", e.scene), e.rt.setup_times())[1],
               lambda e, r: [("rrt_get_setup_times", (SCENE, RT, zeros(e.rrt.CSetupTimes)))])
    stats = dict(kernel_ms=0.5, width=W, height=H, rays_primary=128, scene_bytes=1 << 33, filter_variant=1, origin_plane_triangles=0, filter_pad=0.25,
                 filter_alpha_unit=0.5, filter_delta_unit=0.75)
    yield Case("last_stats", lambda e: e.rt.last_stats(), lambda e, r: [("rrt_last_stats", (RT, zeros(e.rrt.CStats)))],
               replies=lambda e: {"rrt_last_stats": out_fields(1, **stats)}, check=lambda e, r: r == stats)
    yield Case("device_count", lambda e: e.rrt.device_count(), lambda e, r: [("rrt_device_count", (0,))], replies=lambda e: {"rrt_device_count": out_value(0, 8)},
               check=lambda e, r: r == 8)
    yield Case("tiles_per_rank", lambda e: e.rrt.tiles_per_rank(W, H, 2), lambda e, r: [("rrt_tiles_per_rank", (W, H, 2))], status={"rrt_tiles_per_rank": 1},
               check=lambda e, r: r == 1)


def multi_cases():
    yield Case("MultiGpu", lambda e: e.rrt.MultiGpu([e.rt], frames_in_flight=2, loopback=True), lambda e, r: [("rrt_multi_create", ([RT], 1, 2, 1, None))],
               replies=lambda e: {"rrt_multi_create": out_value(4, MULTI)}, check=lambda e, r: r._h.value == MULTI)
    yield Case("MultiGpu(defaults)", lambda e: e.rrt.MultiGpu([e.rt, e.rt]), lambda e, r: [("rrt_multi_create", ([RT, RT], 2, 1, 0, None))])
    yield Case("MultiGpu.dist", lambda e: e.rrt.MultiGpu.dist(e.rt, 1, 2, b"id" * 64, frames_in_flight=3), lambda e, r: [("rrt_dist_create", (RT, 1, 2, b"id" * 64, 3, None))],
               replies=lambda e: {"rrt_dist_create": out_value(5, MULTI)}, check=lambda e, r: r._h.value == MULTI)
    yield Case("MultiGpu.dist(no id)", lambda e: e.rrt.MultiGpu.dist(e.rt, 0, 1, None), lambda e, r: [("rrt_dist_create", (RT, 0, 1, None, 1, None))])
    yield Case("MultiGpu.unique_id", lambda e: e.rrt.MultiGpu.unique_id(), lambda e, r: [("rrt_dist_unique_id", (bytes(128),))],
               replies=lambda e: {"rrt_dist_unique_id": lambda buf: C.memmove(buf, b"\x07" * 128, 128)}, check=lambda e, r: r == b"\x07" * 128)
    yield Case("MultiGpu.render", lambda e: e.mg.render(W, H), lambda e, r: [("rrt_render_multi", (MULTI, W, H, addr(r)))],
               check=lambda e, r: r.shape == (H, W) and r.dtype == np.uint32)
    yield Case("MultiGpu.sync", lambda e: e.mg.sync(), lambda e, r: [("rrt_multi_sync", (MULTI,))])
    yield Case("MultiGpu.last_gather_ms", lambda e: e.mg.last_gather_ms(), lambda e, r: [("rrt_multi_last_gather_ms", (MULTI, -1.0))],
               replies=lambda e: {"rrt_multi_last_gather_ms": out_value(1, 1.5)}, check=lambda e, r: r == 1.5)


CASES = [(c, None) for gen in (creation_cases, scene_data_cases, update_cases, ray_cases, frame_cases, query_cases, multi_cases) for c in gen()]
CASES += [(c, region) for region in (None, REGION) for c in region_cases(region)]


def run(rrt, monkeypatch, case, region, status=None):
    """Runs one case against a fresh recorder: (the Env, the recorder, the result or None, the exception or None)."""
    e = Env(rrt, region)
    rec = Recorder(dict(case.status or {}, **(status or {})), case.replies(e) if case.replies else None)
    monkeypatch.setattr(rrt, "lib", lambda: rec)
    monkeypatch.setattr(rrt, "_lib", rec)                                           # (what a dying object would free its handle with)
    result = error = None
    try:
        result = case.call(e)
    except Exception as x:                                                          # noqa: BLE001 (judged by the caller)
        error = x
    e.made.append(result)                                                           # (the caller ends with e.release())
    return e, rec, result, error


@pytest.mark.parametrize("case,region", CASES, ids=[c.name for c, _ in CASES])
def test_the_call_made(rrt, monkeypatch, case, region):
    e, rec, result, error = run(rrt, monkeypatch, case, region)
    try:
        if case.raises is None:
            assert error is None, repr(error)
        else:
            kind, words = case.raises
            assert type(error).__name__ == (kind if isinstance(kind, str) else kind.__name__) and words in str(error), repr(error)
        want = case.expect(e, result)
        assert [n for n, _ in rec.calls] == [n for n, _ in want]
        for (name, got), (_, args) in zip(rec.calls, want):
            assert len(got) == len(args), (name, got, args)
            for i, (g, a) in enumerate(zip(got, args)):
                assert g == a, f"{name}, argument {i}: got {g!r}, want {a!r}"
        if case.check is not None and error is None:
            assert case.check(e, result)
    finally:
        e.release()


@pytest.mark.parametrize("case,region", [cr for cr in CASES if cr[0].raises is None], ids=[c.name for c, _ in CASES if c.raises is None])
def test_a_refused_call_raises_with_its_status_and_name(rrt, monkeypatch, case, region):
    """Every entry point a case reaches, refused in turn (status -1): RrtError with that status and the entry point's name in its text."""
    e, rec, _, _ = run(rrt, monkeypatch, case, region)
    e.release()
    names = sorted({n for n, _ in rec.calls} - {"rrt_tiles_per_rank"})               # (returns a count, not a status)
    for name in names:
        e, _, _, error = run(rrt, monkeypatch, case, region, status={name: -1})
        e.release()
        assert isinstance(error, rrt.RrtError) and error.status == -1 and name in str(error), (name, repr(error))
        assert "invalid argument" in str(error) and error.detail == "the detail"


def bound_launchers(e):
    return [("rrt_render_device", lambda: e.rt.bind_render(e.t["fb"], W, H, stream=STREAM), (RT, W, H, addr(e.t["fb"]), STREAM)),
            ("rrt_render_tiles_device", lambda: e.rt.bind_render_tiles(e.t["tiles"], W, H, 1, 2, stream=STREAM), (RT, W, H, 1, 2, addr(e.t["tiles"]), STREAM)),
            ("rrt_detile_device", lambda: e.rt.bind_detile(e.t["gathered"], e.t["fb"], W, H, 2, stream=STREAM),
             (RT, W, H, 2, addr(e.t["gathered"]), addr(e.t["fb"]), STREAM)),
            ("rrt_multi_enqueue", lambda: e.mg.bind_enqueue(e.t["fb"], W, H), (MULTI, W, H, addr(e.t["fb"]))),
            ("rrt_multi_enqueue", lambda: e.mg.bind_enqueue(None, W, H), (MULTI, W, H, None))]


def test_bound_launchers_convert_once_and_call_once(rrt, monkeypatch):
    e = Env(rrt, None)
    try:
        for name, bind, args in bound_launchers(e):
            rec = Recorder({"rrt_tiles_per_rank": 1})
            monkeypatch.setattr(rrt, "lib", lambda: rec)
            launch = bind()
            rec.calls.clear(); rec.raw.clear()                                       # (bind time may ask rrt_tiles_per_rank)
            monkeypatch.setattr(rrt, "lib", lambda: pytest.fail("lib() looked up again by a bound launcher"))
            assert launch() is None and launch() is None
            assert rec.calls == [(name, args), (name, args)], name
            first, second = rec.raw[0][1], rec.raw[1][1]
            assert all(a is b for a, b in zip(first, second)), f"{name}: arguments converted again per call"
            assert all(a is None or isinstance(a, (C._SimpleCData, C.Structure)) for a in first), f"{name}: an argument left for ctypes to convert per call"
            monkeypatch.setattr(rrt, "lib", lambda: rec)
            rec.status[name] = -2
            with pytest.raises(rrt.RrtError, match=name) as x:
                launch()
            assert x.value.status == -2
    finally:
        e.release()


def test_bound_launchers_refuse_wrong_tensors(rrt, monkeypatch):
    """What bind_* and the _into forms over them refused before this table existed, they still refuse, by AssertionError and before any launch."""
    e = Env(rrt, None)
    rec = Recorder({"rrt_tiles_per_rank": 1})
    monkeypatch.setattr(rrt, "lib", lambda: rec)
    try:
        for call in (lambda: e.rt.bind_render(e.t["tiles"], W, H, stream=STREAM),                       # 64 elements for 32 pixels
                     lambda: e.rt.bind_render(e.torch.zeros(W * H, dtype=e.torch.int32), W, H, stream=STREAM),     # not on a device
                     lambda: e.rt.render_into(e.dev(e.torch.zeros(W * H, dtype=e.torch.int64)), W, H, stream=STREAM),
                     lambda: e.rt.render_into(e.dev(e.torch.zeros(2 * W * H, dtype=e.torch.int32)[::2]), W, H, stream=STREAM),
                     lambda: e.rt.bind_render_tiles(e.t["fb"], W, H, 0, 2, stream=STREAM),
                     lambda: e.rt.render_tiles_into(e.t["fb"], W, H, 0, 2, stream=STREAM),
                     lambda: e.rt.bind_detile(e.t["tiles"], e.t["fb"], W, H, 2, stream=STREAM),
                     lambda: e.rt.detile_into(e.t["gathered"], e.t["tiles"], W, H, 2, stream=STREAM)):
            with pytest.raises(AssertionError):
                call()
        assert {n for n, _ in rec.calls} <= {"rrt_tiles_per_rank"}
    finally:
        e.release()


def test_tensor_checks_tightened_with_the_marshalling_helpers(rrt, monkeypatch):
    """detile_into / bind_detile checked only element counts and bind_render_tiles not the element size; they now make the common _device_tensor check."""
    e = Env(rrt, None)
    rec = Recorder({"rrt_tiles_per_rank": 1})
    monkeypatch.setattr(rrt, "lib", lambda: rec)
    torch = e.torch
    try:
        for call, words in ((lambda: e.rt.detile_into(torch.zeros(128, dtype=torch.int32), e.t["fb"], W, H, 2, stream=STREAM), "gathered: not a device tensor"),
                            (lambda: e.rt.detile_into(e.t["gathered"], np.zeros(W * H, np.uint32), W, H, 2, stream=STREAM), "fb: not a device tensor"),
                            (lambda: e.rt.bind_detile(e.dev(torch.zeros(128, dtype=torch.int64)), e.t["fb"], W, H, 2, stream=STREAM), "gathered: want 128 contiguous"),
                            (lambda: e.rt.bind_detile(e.t["gathered"], e.dev(torch.zeros(2 * W * H, dtype=torch.int32)[::2]), W, H, 2, stream=STREAM), "fb: want 32 contiguous"),
                            (lambda: e.rt.bind_render_tiles(e.dev(torch.zeros(64, dtype=torch.int64)), W, H, 0, 2, stream=STREAM), "tiles: want 64 contiguous")):
            with pytest.raises(AssertionError, match=words):
                call()
        assert {n for n, _ in rec.calls} <= {"rrt_tiles_per_rank"}
    finally:
        e.release()
