"""Edge values on the GPU against the CPU oracle: texel addressing, bump maps of another size, degenerate shading values, material / light / option
extremes, max_t at its boundary, non-finite rays and non-finite geometry, and a scene loaded end to end from .obj / .mtl / BMP files.

Each case is checked three ways, as tests/test_gpu_lighting.py does, with the checks of tests/gpu_checks.py:
  (a) the default, lane-filter, bundle-filter and ray-walk frames (and get_ray_colours on chosen rays) are bit-identical to the reference-order
      mode (RRT_FLAG_NO_CULL);
  (b) the reference-order frame matches the oracle's: bit for bit where no material evaluates pow() (ks = 0 or ns = -1), else within COLOUR_TOL per
      channel (pow, raytracer.rs:295, may differ by an ulp between glibc and OCML);
  (c) teeth: a count, computed on the host from the oracle's intersect (u, v, triangle) or from the oracle's frames, of the pixels or rays that really
      reach the branch or value the case names, printed and held to a stated minimum.
Where the reference itself would panic -- a NaN box distance in its child sort (ray.rs:147) -- the oracle and the GPU follow the deviation documented
in DESIGN.md ("Non-finite inputs"): NaN is ordered after every number.
"""
import math
import struct

import numpy as np
import pytest

from conftest import channels
from gpu_checks import (ALL_MODES, COLOUR_TOL, N_THREADS, ORIGIN as TEAPOT_ORIGIN, POOL, ROOT_BOX, assert_frame_close, assert_walks_match, check_scene, checker,
                        closed_box, flat_normals, oracle_for, quad, row_dirs)

pytestmark = pytest.mark.gpu
W, H = 96, 72
ORIGIN = (0.0, 0.0, -10.0)                 # hand-built scenes: the plane z = 0 fills the 96 x 72 frame over [-5, 5]^2
INF, NAN = float("inf"), float("nan")


def rust_as_usize(x):
    """Rust `f64 as usize` (raytracer.rs:52-53): NaN and x <= 0 give 0, x >= 2^64 saturates."""
    if not x > 0.0:
        return 0
    return 2**64 - 1 if x >= 2.0**64 else int(x)


def _lights(rrt, spec):
    return [rrt.Light(k, float(i), rrt.Vector3d(*map(float, v))) for k, i, v in spec]


def _exact(materials):
    """No material evaluates pow() (raytracer.rs:286-295): bit equality with the oracle is required."""
    return all(m["ns"] == -1.0 or tuple(m["ks"]) == (0, 0, 0) for m in materials)


def _sample_dirs(w=W, h=H, step=5):
    """Sub-sample directions (engine.rs:207-236) of every `step`-th pixel of every `step`-th row: the chosen rays for get_ray_colours."""
    return np.concatenate([row_dirs(w, h, r, np.arange(0, 2 * (w // 2), step)).reshape(-1, 3) for r in range(1, h, step)])


def primary_hits(osc, origin, w=W, h=H):
    """The oracle's hit (t, u, v, triangle) for sub-sample 0 of every traced pixel: the host side of every teeth count."""
    d = np.concatenate([row_dirs(w, h, r, np.arange(0, 2 * (w // 2)))[0] for r in range(1, h)])
    res = list(POOL.map(lambda v: osc.intersect(origin, v), d))
    return [(d[i],) + r[1:] for i, r in enumerate(res) if r[0]]


def run_case(rrt, ob, name, A, lights, origin=ORIGIN, exact=None, **opt):
    """(a) and (b) for one scene; returns (oracle scene, oracle frame)."""
    exact = _exact(A["materials"]) if exact is None else exact
    tol = 0 if exact else COLOUR_TOL
    sd = rrt.SceneData.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], A["materials"], A["textures"], ROOT_BOX)
    osc = oracle_for(ob, A, lights, origin, **opt)
    V = rrt.Vector3d(*origin)
    ref_rt = rrt.RayTracer(sd, lights, V, no_cull=True, **opt)
    gpu = ref_rt.render(W, H)
    ref = osc.render(W, H, n_threads=N_THREADS)[0]
    d = assert_frame_close(gpu, ref, name, tol)
    D = _sample_dirs()
    O = np.tile(origin, (len(D), 1))
    ref_cols = ref_rt.get_ray_colours(O, D)
    oc = np.fromiter(POOL.map(lambda i: osc.get_ray_colour(O[i], D[i]), range(len(D))), np.uint32, len(D))
    assert_frame_close(ref_cols, oc, f"{name}: get_ray_colours", tol)
    assert_walks_match(lambda mode: rrt.RayTracer(sd, lights, V, box_filter=mode, **opt), [gpu], [(W, H)], name, rays=(O, D, ref_cols))
    print(f"\n[edge] {name}: {(d > 0).sum()} px not bit-equal to the oracle ({'exact' if exact else 'pow'})", end="")
    return osc, ref


def teeth(name, counts, minimum):
    print(f"\n[edge] {name}: teeth " + ", ".join(f"{k} {v} (min {minimum[k]})" for k, v in counts.items()), end="")
    for k, v in counts.items():
        assert v >= minimum[k], f"{name}: only {v} {k} (< {minimum[k]})"


# ------------------------------------------------------------------ scene building
def _panel(x0, x1, y0, y1, z=0.0):
    return quad((x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z))


def _build(panels, materials, textures, nrm=None):
    """panels: [(triangles, material id, uv function (a, b) -> (u, v) over the panel's own [0, 1]^2, or per-triangle uv arrays)]."""
    pos, uv, mat = [], [], []
    for tris, m, f in panels:
        t = np.asarray(tris, np.float64)
        lo, hi = t.reshape(-1, 3).min(0), t.reshape(-1, 3).max(0)
        for k, tri in enumerate(t):
            pos.append(tri); mat.append(m)
            if callable(f):
                a = (tri[:, 0] - lo[0]) / max(hi[0] - lo[0], 1e-30); b = (tri[:, 1] - lo[1]) / max(hi[1] - lo[1], 1e-30)
                uv.append([[*f(a[i], b[i]), 0.0] for i in range(3)])
            else:
                uv.append(np.asarray(f[k], np.float64))
    pos = np.asarray(pos); uv = np.asarray(uv, np.float64); mat = np.asarray(mat, np.uint32)
    nrm = flat_normals(pos, ORIGIN) if nrm is None else np.asarray(nrm, np.float64)
    return dict(pos=pos, uv=uv, nrm=nrm, mat=mat, materials=materials, textures=textures)


def _rand_tex(rng, w, h, lo=1):
    return np.ascontiguousarray(rng.integers(lo, 256, (h, w, 3), dtype=np.uint8))


def _mat(tex, bump=-1, ka=0.3, kd=0.8, ks=0.0, ns=-1.0, kr=0.0):
    v = lambda x: (x, x, x) if np.isscalar(x) else tuple(x)
    return dict(ka=v(ka), kd=v(kd), ks=v(ks), ns=ns, kr=kr, tex=tex, bump=bump)


def _tex_xy(A, tri, u, v):
    """raytracer.rs:43-53 in Python: the raw products tex_x * width, tex_y * height and the texel (x, y) of the colour texture."""
    m = A["materials"][int(A["mat"][tri])]
    tex = A["textures"][m["tex"]]
    th, tw = tex.shape[:2]
    uv = A["uv"][tri]
    w = 1.0 - u - v
    tx = float(uv[1, 0]) * u + float(uv[2, 0]) * v + float(uv[0, 0]) * w
    ty = float(uv[1, 1]) * u + float(uv[2, 1]) * v + float(uv[0, 1]) * w
    rx, ry = tx * float(tw), ty * float(th)
    return (rx, tw, rust_as_usize(rx) % tw), (ry, th, rust_as_usize(ry) % th), m


def _shade_nan(A, tri, u, v):
    """True if get_normal_at_intersection (raytracer.rs:114-162) gives a NaN normal before any bump map: a zero or NaN interpolated normal."""
    nr = A["nrm"][tri]
    w = 1.0 - u - v
    n = [(float(nr[1, k]) * u + float(nr[2, k]) * v) + float(nr[0, k]) * w for k in range(3)]
    return any(math.isnan(c) for c in n) or all(c == 0.0 for c in n)


LIGHTS = ((0, 0.35, (0, 0, 0)), (1, 0.5, (2.0, 3.0, -7.0)), (1, 0.3, (-3.0, -2.0, -5.0)), (2, 0.25, (0.3, 0.4, -1.0)))


# ------------------------------------------------------------------ texel addressing (render.hip umod / f64_as_usize)
TEXEL_SIZES = ((1, 1), (3, 5), (6, 10), (1023, 1), (7, 9), (8, 16))     # (w, h); 8 x 16 is the power-of-two control


def _texel_scene(seed=0x7E1):
    """A 3 x 2 grid of panels at z = 0, one per texture, each cut into four bands whose uv fields send tex * size into one regime each: small
    (with negatives), [2^32, 2^64), beyond 2^64 / +inf, and NaN (from a NaN uv, or inf * 0 at a vertex)."""
    rng = np.random.default_rng(seed)
    textures = [_rand_tex(rng, w, h) for w, h in TEXEL_SIZES]
    materials = [_mat(i) for i in range(len(textures))]
    bands = [lambda a, b: (a * 6.3 - 1.7, b * 9.1 - 2.2),
             lambda a, b: (2.0**34 + a * 5000.3, 3e9 + b * 777.7),
             lambda a, b: (1e25 * (1.0 + a), 2.0**64 * (1.0 + b)),
             None]
    panels = []
    for i in range(6):
        cx, y0 = -3.3 + 3.3 * (i % 3), (0.05 if i < 3 else -4.95)
        for k, f in enumerate(bands):
            tris = _panel(cx - 1.6, cx + 1.6, y0 + 1.225 * k, y0 + 1.225 * (k + 1))
            if f is None:         # one triangle with a NaN uv at a vertex, one with +inf at two vertices: inf * u + inf * v + f * w, NaN where u = 0
                f = [[[NAN, 0.3, 0], [0.1, 0.2, 0], [0.4, 0.5, 0]], [[0.25, 0.75, 0], [INF, INF, 0], [INF, -INF, 0]]]
            panels.append((tris, i, f))
    return _build(panels, materials, textures)


def test_texel_addressing_non_power_of_two(rrt, ob):
    A = _texel_scene()
    lights = _lights(rrt, LIGHTS)
    osc, _ = run_case(rrt, ob, "texel addressing", A, lights)
    n = dict(mask=0, mod32=0, mod64=0, saturated_or_nan=0)
    for d, t, u, v, tri in primary_hits(osc, ORIGIN):
        for raw, size, _ in _tex_xy(A, tri, u, v)[:2]:
            if size & (size - 1) == 0:
                n["mask"] += 1
            elif math.isnan(raw) or raw >= 2.0**64:
                n["saturated_or_nan"] += 1
            elif rust_as_usize(raw) <= 0xFFFFFFFF:
                n["mod32"] += 1
            else:
                n["mod64"] += 1
    teeth("texel addressing (umod branch per hit axis)", n, dict(mask=300, mod32=300, mod64=300, saturated_or_nan=300))


# ------------------------------------------------------------------ bump maps
def _bump_scene(seed=0xB0B):
    """Panels: a bump map wider than its 3 x 2 colour texture; one narrower but taller (its index wraps into the next row); one holding black texels;
    one exactly fitting (8 x 3 colour, 4 x 4 bump: the last texel is addressed); vertex normals exactly (0, +-1, 0) under a bump map (the tangent
    fallback, raytracer.rs:143-149); a bump-mapped mirror with black texels (NaN reflection and shadow rays)."""
    rng = np.random.default_rng(seed)
    col32 = _rand_tex(rng, 3, 2)
    black = _rand_tex(rng, 4, 4); black[::2, ::2] = 0; black[1, 2] = 0
    textures = [col32, _rand_tex(rng, 5, 2), _rand_tex(rng, 2, 4), _rand_tex(rng, 4, 4), black, _rand_tex(rng, 8, 3), _rand_tex(rng, 4, 4),
                _rand_tex(rng, 6, 5)]
    materials = [_mat(0, bump=1), _mat(0, bump=2), _mat(3, bump=4), _mat(5, bump=6), _mat(0, bump=7, ka=0.5), _mat(3, bump=4, kr=0.5, ka=0.4)]
    uvf = lambda a, b: (a * 2.3 - 0.15, b * 1.7 + 0.05)
    panels = [(_panel(-4.9, -1.75, 0.05, 4.9), 0, uvf), (_panel(-1.6, 1.6, 0.05, 4.9), 1, uvf), (_panel(1.75, 4.9, 0.05, 4.9), 2, uvf),
              (_panel(-4.9, -1.75, -4.9, -0.05), 3, lambda a, b: (a * 0.999, b * 0.999)), (_panel(-1.6, 1.6, -4.9, -0.05), 4, uvf)]
    mirror = quad((1.75, -4.9, -1.5), (4.9, -4.9, 0.5), (4.9, -0.05, 0.5), (1.75, -0.05, -1.5))      # turned towards the other panels
    panels.append((mirror, 5, uvf))
    back = _panel(-12.0, 12.0, -12.0, 12.0, z=-11.0)                                                   # behind the camera: what the mirror shows
    panels.append((back, 4, uvf))
    A = _build(panels, materials, textures)
    fb = np.flatnonzero(A["mat"] == 4)[:2]                                                             # the (0, +-1, 0) panel's two triangles
    A["nrm"][fb[0]] = [0.0, 1.0, 0.0]; A["nrm"][fb[1]] = [0.0, -1.0, 0.0]
    return A


def _bump_texels(A, tri, u, v):
    """(texel the reference reads: colour (x, y), bump width; texel at the bump map's own (x, y)) for a hit on a bump-mapped material."""
    (rx, tw, xi), (ry, th, yi), m = _tex_xy(A, tri, u, v)
    b = A["textures"][m["bump"]]
    bh, bw = b.shape[:2]
    k = bw * yi + xi
    own = (rust_as_usize(ry / th * bh) % bh, rust_as_usize(rx / tw * bw) % bw)
    return b[k // bw, k % bw], b[own], m, A["textures"][m["tex"]].shape[:2], (bh, bw)


def test_bump_maps(rrt, ob):
    A = _bump_scene()
    lights = _lights(rrt, LIGHTS)
    osc, _ = run_case(rrt, ob, "bump maps", A, lights)
    n = dict(wider=0, narrower_taller_wrapped=0, own_xy_differs=0, black_texel=0, tangent_fallback=0, exact_fit_last_texel=0, nan_mirror=0)
    for d, t, u, v, tri in primary_hits(osc, ORIGIN):
        m = A["materials"][int(A["mat"][tri])]
        if m["bump"] < 0:
            continue
        got, own, m, (th, tw), (bh, bw) = _bump_texels(A, tri, u, v)
        (_, _, xi), (_, _, yi), _ = _tex_xy(A, tri, u, v)
        n["wider"] += bw > tw
        n["narrower_taller_wrapped"] += bw < tw and bh > th and (bw * yi + xi) // bw != yi
        n["own_xy_differs"] += bool((got != own).any())
        n["black_texel"] += bool((got == 0).all())
        nr = A["nrm"][tri]
        n["tangent_fallback"] += bool((nr[:, 0] == 0).all() and (nr[:, 2] == 0).all())
        n["exact_fit_last_texel"] += (th, tw) == (3, 8) and bw * yi + xi == bw * bh - 1
        n["nan_mirror"] += m["kr"] > 0 and bool((got == 0).all())
    teeth("bump maps (primary hits)", n, dict(wider=300, narrower_taller_wrapped=100, own_xy_differs=1000, black_texel=200, tangent_fallback=300,
                                              exact_fit_last_texel=20, nan_mirror=30))


def test_bump_map_size_check(rrt):
    """validate_tables (api.cpp; validate_model and rrt_raytracer_create_from_arrays both go through it): the bump index bump.width * y + x (raytracer.rs:127-128) over every colour texel must stay inside the bump map.  An 8 x 3
    colour texture addresses up to 4 * 2 + 7 = 15 in a 4-wide bump map: 4 x 4 fits exactly; a 9 x 3 colour texture (index 16) is one texel short."""
    tri = np.array([[[-1, 0, 2], [1, 0, 2], [0, 1, 2]]], np.float64)
    uv = np.zeros((1, 3, 3)); nrm = np.tile([0.0, 0.0, -1.0], (1, 3, 1))
    mats = [_mat(0, bump=1)]
    bump = np.full((4, 4, 3), 90, np.uint8)
    rrt.SceneData.from_arrays(tri, uv, nrm, np.zeros(1, np.uint32), mats, [np.zeros((3, 8, 3), np.uint8), bump])
    for colour in (np.zeros((3, 9, 3), np.uint8), np.zeros((4, 5, 3), np.uint8)):      # index 16; 4 * 3 + 4 = 16
        with pytest.raises(rrt.RrtError) as e:
            rrt.SceneData.from_arrays(tri, uv, nrm, np.zeros(1, np.uint32), mats, [colour, bump])
        assert e.value.status == rrt.ERR_INVALID_ARG


# ------------------------------------------------------------------ degenerate shading normals
def _degenerate_scene(seed=0xDE6):
    rng = np.random.default_rng(seed)
    textures = [_rand_tex(rng, 4, 4), _rand_tex(rng, 5, 3), checker((200, 200, 200), (60, 90, 120), 4)]
    materials = [_mat(0), _mat(1, kr=0.5, ka=0.4), _mat(2, kd=0.9)]
    uvf = lambda a, b: (a * 1.3, b * 0.9)
    panels = [(_panel(-4.9, -1.75, 0.05, 4.9), 0, uvf), (_panel(-1.6, 1.6, 0.05, 4.9), 0, uvf), (_panel(1.75, 4.9, 0.05, 4.9), 0, uvf),
              (quad((-4.9, -4.9, -1.0), (-1.75, -4.9, 1.0), (-1.75, -0.05, 1.0), (-4.9, -0.05, -1.0)), 1, uvf),       # mirrors
              (quad((-1.6, -4.9, 1.0), (1.6, -4.9, -1.0), (1.6, -0.05, -1.0), (-1.6, -0.05, 1.0)), 1, uvf),
              (_panel(1.75, 4.9, -4.9, -0.05), 2, uvf),
              (closed_box((1.0, 1.0, -4.0), (2.0, 2.0, -3.0)), 2, uvf),                                              # an occluder for the point light
              (_panel(-12.0, 12.0, -12.0, 12.0, z=-11.0), 2, uvf)]
    A = _build(panels, materials, textures)
    nrm = A["nrm"]
    z, c, q = [np.flatnonzero(A["mat"] == 0)[i:i + 2] for i in (0, 2, 4)]
    nrm[z] = 0.0                                                                         # zero vertex normals: normalised(0) = NaN
    nrm[c] = [[0.0, 0.0, -1.0], [0.0, 0.0, 1.0], [0.6, 0.0, 0.0]]                        # normals that cancel inside the triangle
    nrm[q, 0, 0] = NAN                                                                   # a NaN component
    mir = np.flatnonzero(A["mat"] == 1)
    nrm[mir[0]] = 0.0                                                                    # a mirror with zero normals: NaN reflection rays
    nrm[mir[2]] = [[0.0, 0.0, -1.0], [0.0, 0.0, 1.0], [0.0, 0.0, -1.0]]
    nrm[mir[3], 1, 2] = NAN
    return A


def test_degenerate_normals(rrt, ob):
    A = _degenerate_scene()
    lights = _lights(rrt, LIGHTS)
    osc, _ = run_case(rrt, ob, "degenerate normals", A, lights)
    n = dict(nan_normal=0, nan_shadow_rays=0, nan_reflection=0, flipped_normal=0)
    for d, t, u, v, tri in primary_hits(osc, ORIGIN):
        m = A["materials"][int(A["mat"][tri])]
        if _shade_nan(A, tri, u, v):
            n["nan_normal"] += 1
            n["nan_shadow_rays"] += 1                                    # the first point light's shadow ray starts at p + NaN
            n["nan_reflection"] += m["kr"] > 0
        else:
            nr = A["nrm"][tri]; w = 1.0 - u - v
            nz = (nr[1, 2] * u + nr[2, 2] * v) + nr[0, 2] * w
            n["flipped_normal"] += bool(nz > 0 and (nr[:, 2] < 0).any())
    teeth("degenerate normals (primary hits)", n, dict(nan_normal=1000, nan_shadow_rays=1000, nan_reflection=200, flipped_normal=100))


# ------------------------------------------------------------------ material, light and option extremes
def _extreme_scene(floor=None, wall=None, mirror=None, box=None):
    """Floor, back wall, a mirror turned towards them and a closed box; each material's values can be replaced."""
    rng = np.random.default_rng(0xE7)
    textures = [checker((200, 180, 150), (90, 110, 140)), _rand_tex(rng, 5, 3), checker((230, 230, 230), (40, 60, 80), 4), _rand_tex(rng, 3, 7)]
    base = [_mat(0, ka=0.6, kd=0.8, ks=0.5, ns=20.0), _mat(1, ka=0.5, kd=0.7), _mat(2, ka=0.6, kd=0.5, kr=0.6), _mat(3, ka=0.7, kd=0.9, ks=0.6, ns=8.0)]
    for m, over in zip(base, (floor, wall, mirror, box)):
        m.update(over or {})
    uvf = lambda a, b: (a * 2.1, b * 1.3)
    panels = [(quad((-6, -3, -4), (6, -3, -4), (6, -3, 8), (-6, -3, 8)), 0, uvf),
              (_panel(-6, 6, -3, 6, z=8.0), 1, uvf),
              (quad((2.5, -3, -2), (6, -3, 3), (6, 4, 3), (2.5, 4, -2)), 2, uvf),
              (closed_box((-3.0, -3.0, 1.0), (-1.0, -1.0, 3.0)), 3, uvf)]
    A = _build(panels, base, textures)
    A["nrm"] = flat_normals(A["pos"], (0.0, 0.0, 0.0))
    return A


NEXT_M1 = math.nextafter(-1.0, 0.0)
BASE_LIGHTS = ((0, 0.3, (0, 0, 0)), (1, 0.5, (-4.0, 4.0, -6.0)), (1, 0.3, (3.0, 5.0, 0.0)), (2, 0.2, (0.5, 1.0, -1.0)))
# name: (material overrides per (floor, wall, mirror, box), lights, options, neighbour (overrides, lights, options), minimum teeth in pixels)
EXTREMES = {
    "ns_sentinel_-1": (({"ns": -1.0}, None, None, {"ns": -1.0}), BASE_LIGHTS, {}, (({"ns": NEXT_M1}, None, None, {"ns": NEXT_M1}), None, None), 500),
    "ns_nextafter_-1": (({"ns": NEXT_M1}, None, None, {"ns": NEXT_M1}), BASE_LIGHTS, {}, (({"ns": -1.0}, None, None, {"ns": -1.0}), None, None), 500),
    "ns_-5": (({"ns": -5.0}, None, None, {"ns": -5.0}), BASE_LIGHTS, {}, (({"ns": -1.0}, None, None, {"ns": -1.0}), None, None), 500),
    "ns_0": (({"ns": 0.0}, None, None, {"ns": 0.0}), BASE_LIGHTS, {}, (({"ns": -1.0}, None, None, {"ns": -1.0}), None, None), 500),
    "ns_inf": (({"ns": INF}, None, None, {"ns": INF}), BASE_LIGHTS, {}, (({"ns": 0.0}, None, None, {"ns": 0.0}), None, None), 500),
    "ns_nan": (({"ns": NAN}, None, None, {"ns": NAN}), BASE_LIGHTS, {}, (({"ns": -1.0}, None, None, {"ns": -1.0}), None, None), 500),
    "kr_1_infinite_local": ((None, None, {"kr": 1.0}, None), ((0, INF, (0, 0, 0)),) + BASE_LIGHTS[1:], {}, ((None, None, {"kr": 0.5}, None), None, None), 200),
    "kr_1": ((None, None, {"kr": 1.0}, None), BASE_LIGHTS, {}, ((None, None, {"kr": 0.5}, None), None, None), 200),
    "kr_1.5": ((None, None, {"kr": 1.5}, None), BASE_LIGHTS, {}, ((None, None, {"kr": 0.5}, None), None, None), 200),
    "kr_-0.5": ((None, None, {"kr": -0.5}, None), BASE_LIGHTS, {}, ((None, None, {"kr": 0.5}, None), None, None), 200),
    "kr_nan": ((None, None, {"kr": NAN}, None), BASE_LIGHTS, {}, ((None, None, {"kr": 0.5}, None), None, None), 200),
    "kr_denormal": ((None, None, {"kr": 5e-324}, None), BASE_LIGHTS, {}, ((None, None, {"kr": 0.5}, None), None, None), 200),
    "ka_kd_ks_nonfinite": (({"kd": (NAN, 1.0, INF)}, {"ka": (INF, -INF, NAN)}, None, {"ks": (INF, 0.0, -INF)}), BASE_LIGHTS, {}, ((None,) * 4, None, None), 500),
    "intensity_inf": ((None,) * 4, ((0, 0.3, (0, 0, 0)), (1, INF, (-4.0, 4.0, -6.0)), (2, -INF, (0.5, 1.0, -1.0))), {}, ((None,) * 4, None, None), 500),
    "intensity_nan": ((None,) * 4, ((0, NAN, (0, 0, 0)), (1, 0.5, (-4.0, 4.0, -6.0)), (2, 0.2, (0.5, 1.0, -1.0))), {}, ((None,) * 4, None, None), 500),
    "point_at_inf": ((None,) * 4, ((0, 0.3, (0, 0, 0)), (1, 0.5, (INF, 0.0, 0.0)), (1, 0.3, (3.0, 5.0, 0.0))), {}, ((None,) * 4, None, None), 500),
    "point_at_nan": ((None,) * 4, ((0, 0.3, (0, 0, 0)), (1, 0.5, (NAN, 1.0, 1.0)), (1, 0.3, (3.0, 5.0, 0.0))), {}, ((None,) * 4, None, None), 500),
    "point_at_inf3": ((None,) * 4, ((1, 0.5, (INF, INF, INF)), (0, 0.3, (0, 0, 0))), {}, ((None,) * 4, None, None), 500),
    "directional_inf_nan": ((None,) * 4, ((0, 0.3, (0, 0, 0)), (2, 0.5, (INF, INF, INF)), (2, 0.4, (NAN, 0.0, 1.0))), {}, ((None,) * 4, None, None), 500),
    "surface_offset_nan": ((None,) * 4, BASE_LIGHTS, {"surface_offset": NAN}, ((None,) * 4, None, {"surface_offset": 1e-4}), 500),
    "surface_offset_-1e-4": ((None,) * 4, BASE_LIGHTS, {"surface_offset": -1e-4}, ((None,) * 4, None, {"surface_offset": 1e-2}), 20),
}


@pytest.mark.parametrize("case", list(EXTREMES))
def test_material_light_option_extremes(rrt, ob, case):
    """The API validates none of these values, and none needs refusing: each renders as the reference computes it (NaN -> 0 and +inf -> 255 in
    clamp_u8, inf * 0 = NaN -> black under kr = 1, ns = -1 alone switches specular off, a NaN max_t or offset misses everything)."""
    over, lights, opt, (n_over, n_lights, n_opt), min_teeth = EXTREMES[case]
    A = _extreme_scene(*over)
    osc, ref = run_case(rrt, ob, case, A, _lights(rrt, lights), **opt)
    nA = _extreme_scene(*n_over)
    nref = oracle_for(ob, nA, _lights(rrt, n_lights or BASE_LIGHTS), ORIGIN, **(opt if n_opt is None else n_opt)).render(W, H, n_threads=N_THREADS)[0]
    if case == "kr_denormal":                         # 1 - 5e-324 == 1: the frame equals kr = 0's, but every mirror hit traces its reflection
        hits = sum(int(A["mat"][h[4]]) == 2 for h in primary_hits(osc, ORIGIN))
        teeth(case, {"mirror hits (reflection traced)": hits}, {"mirror hits (reflection traced)": min_teeth})
        kr0 = oracle_for(ob, _extreme_scene(None, None, {"kr": 0.0}, None), _lights(rrt, lights), ORIGIN).render(W, H, n_threads=N_THREADS)[0]
        assert np.array_equal(ref, kr0)
        return
    diff = int((nref != ref).sum())
    teeth(case, {"pixels differing from the neighbouring configuration": diff}, {"pixels differing from the neighbouring configuration": min_teeth})
    if case == "kr_1_infinite_local":                 # inf * (1 - 1) = NaN -> 0 in every channel of every mirror pixel
        assert (ref == 0).sum() >= min_teeth


# ------------------------------------------------------------------ max_t at its boundary
@pytest.fixture(scope="module")
def boundary_rays(teapot, teapot_oracle):
    """Rays from scattered origins whose oracle hit has t = T, with T and whether the hit triangle is in the root's own list."""
    rng = np.random.default_rng(0x3A7)
    n = 7000
    o = rng.uniform([-7, -1, -9], [7, 7, 7], (n, 3)); d = rng.normal(size=(n, 3))
    d[::2] = rng.uniform([-2.5, 0.0, -2.0], [2.5, 3.0, 2.0], (n // 2, 3)) - o[::2]          # half of them towards the teapot: hits in children
    res = list(POOL.map(lambda i: teapot_oracle.intersect(o[i], d[i]), range(n)))
    keep = [i for i, r in enumerate(res) if r[0]][:2500]
    tree = teapot_oracle.octree()
    root = set(tree["own_idx"][tree["own_off"][0]:tree["own_off"][1]].tolist())
    T = np.array([res[i][1] for i in keep])
    from_root = np.array([res[i][4] in root for i in keep])
    return o[keep], d[keep], T, from_root


def test_max_t_boundary(rrt, teapot, teapot_oracle, boundary_rays):
    O, D, T, from_root = boundary_rays
    assert len(O) >= 2000
    variants = {"T": T, "next_up": np.nextafter(T, INF), "next_down": np.nextafter(T, -INF), "nan": NAN, "0": 0.0, "-0": -0.0, "-1": -1.0,
                "-inf": -INF, "5e-324": 5e-324}
    rts = {"no_cull": rrt.RayTracer(teapot, rrt.default_lights(), no_cull=True)}
    rts.update({str(m): rrt.RayTracer(teapot, rrt.default_lights(), box_filter=m) for m in ALL_MODES})
    changed = 0
    for name, mt in variants.items():
        M = np.broadcast_to(np.asarray(mt, np.float64), (len(O),))
        ref = list(POOL.map(lambda i: teapot_oracle.intersect(O[i], D[i], M[i]), range(len(O))))
        rh = np.array([r[0] for r in ref])
        if name == "T":
            changed = int((~rh).sum() + sum(r[0] and r[1] != t for r, t in zip(ref, T)))
        if name not in ("T", "next_up", "next_down"):
            assert not rh.any(), f"oracle: max_t {name} must miss every ray (nothing is < it but its own hits, ray.rs:117-129, 163)"
        for mode, rt in rts.items():
            hit, t, u, v, tri = rt.intersect_rays(O, D, M)
            assert np.array_equal(hit, rh), f"max_t {name}, walk {mode}: {(hit != rh).sum()} rays differ in hit/miss from the oracle"
            for i in np.flatnonzero(rh):
                assert (t[i], u[i], v[i], tri[i]) == ref[i][1:], f"max_t {name}, walk {mode}, ray {i}: ({t[i]!r}, {u[i]!r}, {v[i]!r}, {tri[i]}) vs {ref[i][1:]}"
    n = {"boundary hits from the root's own list": int(from_root.sum()), "boundary hits from a child": int((~from_root).sum()),
         "rays whose answer changes at max_t = T": changed}
    teeth("max_t boundary", n, {"boundary hits from the root's own list": 100, "boundary hits from a child": 500, "rays whose answer changes at max_t = T": 1000})


# ------------------------------------------------------------------ non-finite rays
def _special_rays():
    """NaN / +inf / -inf in each component of the origin and of the direction, the zero direction and the direction (inf, inf, inf)."""
    o0, d0 = np.array(TEAPOT_ORIGIN), np.array([0.05, -0.08, 1.0])
    O, D = [], []
    for val in (NAN, INF, -INF):
        for k in range(3):
            o = o0.copy(); o[k] = val; O.append(o); D.append(d0)
            d = d0.copy(); d[k] = val; O.append(o0); D.append(d)
    O += [o0, o0, np.array([INF, INF, INF]), np.array([1.0, 1.0, -8.0])]
    D += [np.zeros(3), np.array([INF, INF, INF]), d0, np.array([NAN, NAN, NAN])]
    return np.array(O), np.array(D)


@pytest.fixture(scope="module")
def ordinary_rays():
    rng = np.random.default_rng(0x0DD)
    n = 64 * 1024 + 1
    o = rng.uniform([-7, -1, -9], [7, 7, 7], (n, 3)); d = rng.normal(size=(n, 3))
    o[::2] = TEAPOT_ORIGIN; d[::2] = np.stack([rng.uniform(-0.5, 0.5, (n + 1) // 2), rng.uniform(-0.5, 0.5, (n + 1) // 2), np.ones((n + 1) // 2)], -1)
    return o, d


def test_non_finite_rays(rrt, teapot, teapot_oracle, ordinary_rays):
    SO, SD = _special_rays()
    ns = len(SO)
    ref_hit = [teapot_oracle.intersect(SO[i], SD[i]) for i in range(ns)]
    ref_col = np.array([teapot_oracle.get_ray_colour(SO[i], SD[i]) for i in range(ns)], np.uint32)
    OO, OD = ordinary_rays
    k = 1500
    ord_hit = list(POOL.map(lambda i: teapot_oracle.intersect(OO[i], OD[i]), range(k)))
    ord_col = np.fromiter(POOL.map(lambda i: teapot_oracle.get_ray_colour(OO[i], OD[i]), range(k)), np.uint32, k)
    rts = {"no_cull": rrt.RayTracer(teapot, rrt.default_lights(), no_cull=True)}
    rts.update({str(m): rrt.RayTracer(teapot, rrt.default_lights(), box_filter=m) for m in ALL_MODES})
    n_mixed = 0
    for mode, rt in rts.items():
        base_hit, base_t, base_u, base_v, base_tri = rt.intersect_rays(OO, OD)
        base_col = rt.get_ray_colours(OO, OD)
        for i in range(k):                                           # the ordinary rays alone against the oracle
            assert bool(base_hit[i]) == ord_hit[i][0] and (not ord_hit[i][0] or (base_t[i], base_u[i], base_v[i], base_tri[i]) == ord_hit[i][1:]), (mode, i)
        assert_frame_close(base_col[:k], ord_col, f"walk {mode}: ordinary ray colours")
        for n in (1, 63, 65, 64 * 1024 + 1):
            slots = [np.array([s]) for s in range(ns)] if n == 1 else [np.linspace(0, n - 1, ns).astype(np.int64)]
            for pos in slots:
                O, D = OO[:n].copy(), OD[:n].copy()
                if n == 1:                                           # one special ray on its own
                    sp, where = pos, np.arange(1)
                else:                                                # all of them, spread through the batch
                    sp, where = np.arange(ns), pos
                O[where], D[where] = SO[sp], SD[sp]
                hit, t, u, v, tri = rt.intersect_rays(O, D)
                col = rt.get_ray_colours(O, D)
                for j, s in zip(where, sp):
                    rh = ref_hit[s]
                    assert bool(hit[j]) == rh[0] and (not rh[0] or (t[j], u[j], v[j], tri[j]) == rh[1:]), (mode, n, s, hit[j], t[j], rh)
                    assert np.abs(channels(col[j]) - channels(ref_col[s])).max() <= COLOUR_TOL, (mode, n, s, hex(col[j]), hex(ref_col[s]))
                rest = np.ones(len(O), bool); rest[where] = False
                assert np.array_equal(hit[rest], base_hit[:n][rest]) and np.array_equal(tri[rest], base_tri[:n][rest]), (mode, n)
                assert np.array_equal(t[rest], base_t[:n][rest]) and np.array_equal(u[rest], base_u[:n][rest]) and np.array_equal(v[rest], base_v[:n][rest]), (mode, n)
                assert np.array_equal(col[rest], base_col[:n][rest]), (mode, n)
                n_mixed += n > 1
    waves = {n: len({int(p) // 64 for p in np.linspace(0, n - 1, ns).astype(np.int64)}) for n in (63, 65, 64 * 1024 + 1)}
    teeth("non-finite rays", {"special rays": ns, "mixed batches": n_mixed, "waves of 65 holding a special ray": waves[65]},
          {"special rays": 20, "mixed batches": 15, "waves of 65 holding a special ray": 2})


# ------------------------------------------------------------------ non-finite geometry
def test_non_finite_geometry(rrt, ob):
    """Triangles with NaN or infinite vertices among ordinary ones.  The reference builds such a tree without complaint (f64::min / max ignore NaN,
    aabb.rs:25-47; a NaN comparison makes aabb.rs:49-60 report an overlap), and its ray tests never hit them (a NaN reaches `t > EPSILON` as false,
    ray.rs:89): the GPU build must equal the host build and the oracle's tree, and the frames must equal the oracle's."""
    A = _extreme_scene()
    bad = np.array([[(NAN, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)],
                    [(INF, 1.0, 2.0), (1.0, 1.0, 2.0), (1.0, 2.0, 2.0)],
                    [(-INF, -INF, -INF), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)],
                    [(NAN, NAN, NAN)] * 3,
                    [(0.5, -1.0, INF), (1.5, -1.0, 4.0), (0.5, 0.0, 4.0)],
                    [(-2.0, 0.0, 5.0), (NAN, 1.0, 5.0), (-2.0, 1.0, INF)]])
    at = [3, 9, 17]                                                 # spread through the push order
    pos = np.insert(A["pos"], at, bad[:3], 0); pos = np.concatenate([pos, bad[3:]])
    nb = len(pos) - len(A["pos"])
    A = dict(A, pos=pos, uv=np.concatenate([A["uv"], np.zeros((nb, 3, 3))]), nrm=np.concatenate([A["nrm"], np.tile([0.0, 0.0, -1.0], (nb, 3, 1))]),
             mat=np.concatenate([A["mat"], np.zeros(nb, np.uint32)]))
    sd = rrt.SceneData.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], A["materials"], A["textures"], ROOT_BOX)
    check_scene(rrt, sd, "non-finite geometry", ob)
    osc, _ = run_case(rrt, ob, "non-finite geometry", A, _lights(rrt, BASE_LIGHTS))
    bad_ids = {i for i in range(len(pos)) if not np.isfinite(pos[i]).all()}
    tree = osc.octree()
    in_tree = len(bad_ids & set(tree["own_idx"].tolist()))
    hits = primary_hits(osc, ORIGIN)
    assert not any(h[4] in bad_ids for h in hits)
    teeth("non-finite geometry", {"non-finite triangles in the tree": in_tree, "primary hits": len(hits)},
          {"non-finite triangles in the tree": 4, "primary hits": 3000})


# ------------------------------------------------------------------ the loader end to end
def _bmp(img):
    """24-bit uncompressed BMP: bottom-up rows of BGR, each padded to 4 bytes."""
    h, w = img.shape[:2]
    row = (3 * w + 3) & ~3
    px = b"".join(img[r, :, ::-1].tobytes() + b"\0" * (row - 3 * w) for r in range(h - 1, -1, -1))
    return b"BM" + struct.pack("<IHHI", 54 + len(px), 0, 0, 54) + struct.pack("<IiiHHIIiiII", 40, w, h, 1, 24, 0, len(px), 2835, 2835, 0, 0) + px


def test_loader_end_to_end(rrt, ob, tmp_path):
    rng = np.random.default_rng(0x10AD)
    tex, bump = _rand_tex(rng, 37, 23), _rand_tex(rng, 37, 23, lo=20)
    (tmp_path / "t.bmp").write_bytes(_bmp(tex)); (tmp_path / "b.bmp").write_bytes(_bmp(bump))
    (tmp_path / "s.mtl").write_text("newmtl plain\nKa 0.4 0.4 0.4\nKd 0.8 0.7 0.6\nKs 0 0 0\nNs 12\nmap_Ka t.bmp\nbump b.bmp\n"
                                    "newmtl mirror\nKa 0.5 0.5 0.5\nKd 0.6 0.6 0.6\nKs 0 0 0\nKr 0.5\nmap_Ka t.bmp\n")
    lines = ["mtllib s.mtl"]
    lines += [f"v {x} {y} {z}" for x, y, z in ((-5, -5, 0), (5, -5, 0), (5, 5, 0), (-5, 5, 0), (1, -4, -3), (4, -4, -1), (4, 2, -1), (1, 2, -3),
                                               (-9, -9, -11), (9, -9, -11), (9, 9, -11), (-9, 9, -11))]
    lines += [f"vt {u} {v}" for u, v in ((0, 0), (1.7, 0), (1.7, 1.3), (0, 1.3), (-0.2, 0.1), (2.9, 0.4))]
    lines += ["vn 0 0 -1", "vn 0.3 0.2 -1", "vn -0.5 0.8 -0.6", "vn 0 0 1"]
    lines += ["usemtl plain", "f 1/1/1 2/2/2 3/3/1", "f 1/1/1 3/3/3 4/4/2", "f 9/5/4 10/6/4 11/3/4", "f 9/5/4 11/3/4 12/1/4",
              "usemtl mirror", "f 5/1/2 6/2/1 7/3/3", "f 5/1/2 7/3/3 8/4/1"]
    (tmp_path / "s.obj").write_text("\n".join(lines) + "\n")
    sd = rrt.parse_obj_file(str(tmp_path / "s.obj"))
    got = sd.textures()
    assert len(got) == 2 and np.array_equal(got[0], tex) and np.array_equal(got[1], bump)
    pos, uv, nrm, mat = sd.triangles()
    A = dict(pos=pos, uv=uv, nrm=nrm, mat=mat, materials=sd.materials(), textures=got)
    assert A["materials"][0]["bump"] == 1 and A["materials"][1]["kr"] == 0.5 and len(pos) == 6
    osc, _ = run_case(rrt, ob, "loader end to end", A, _lights(rrt, LIGHTS))
    hits = primary_hits(osc, ORIGIN)
    n = {"bump-mapped hits": sum(A["materials"][int(mat[h[4]])]["bump"] >= 0 for h in hits),
         "mirror hits": sum(A["materials"][int(mat[h[4]])]["kr"] > 0 for h in hits)}
    teeth("loader end to end", n, {"bump-mapped hits": 2000, "mirror hits": 500})
