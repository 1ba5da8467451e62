"""Helpers shared by the surface-buffer tests (include/rrt.h: rrt_render_surface): the expected planes, restated on the host from the reference.

Plain module, not a test module: pytest does not rewrite its asserts, so every assert here states both values in its message.  It holds no fixtures.

The oracle exports an intersector and a shader, not the normal or the light loop's intermediate results, so the part of the reference between the two is
restated here in numpy, one rounded f64 operation per reference operation and in its order:
    raytracer.rs:39-57    hit point, barycentric texture coordinates, saturating `as usize`, texel indices
    raytracer.rs:114-162  get_normal_at_intersection (interpolation, bump map through the tangent frame, normalisation)
    raytracer.rs:164-188  triangle_exists_between_points: the shadow ray; Some/None of it is asked of the oracle's intersector
t, u, v and the triangle come from the oracle's intersector.  numpy's elementwise +, -, *, / and sqrt are IEEE operations, each rounded once and never
fused; sums are written with the reference's parentheses.  No np.dot, np.cross, np.linalg.norm or einsum: their summation order is not the reference's.
`shade` goes on from the planes to colours (raytracer.rs:192-304, 67-108) and is what shows that the restatement is the reference's: on the CPU it reproduces
the oracle's get_ray_colour on every non-mirror hit of the teapot frames with zero channel difference.
"""
import numpy as np

from bitwise import same
from gpu_checks import POOL, pose_dirs, traced_rows

NO_MATERIAL = 0xFFFFFFFF
MISS = dict(point=0.0, normal=0.0, material=NO_MATERIAL, lights=0)          # a miss and a pixel the reference never traces, rrt.h
VIS_NEVER_TRACED = dict(hit=0, t=0.0, u=0.0, v=0.0, tri=0xFFFFFFFF, albedo=0)


# ------------------------------------------------------------------ the frame's rays
def traced_cols(w):
    return np.arange(2 * (w // 2))


def frame_dirs(cam, w, h, viewport=(1.0, 1.0, 1.0)):
    """[len(rows)][len(cols)][4][3]: directions of the traced pixels' sub-sample rays, in the planes' index order."""
    return pose_dirs(cam, w, h, traced_rows(h), traced_cols(w), viewport).transpose(0, 2, 1, 3)


def traced_part(planes, w, h):
    ix = np.ix_(traced_rows(h), traced_cols(w))
    return {n: a[ix] for n, a in planes.items()}


def traced_pixels_in(region, w, h):
    x0, y0, rw, rh = region
    rows, cols = traced_rows(h), traced_cols(w)
    return int(((rows >= y0) & (rows < y0 + rh)).sum()) * int(((cols >= x0) & (cols < x0 + rw)).sum())


def assert_untraced_pixels(planes, w, h, what):
    """Row 0, row 1 of an odd height and the last column of an odd width hold the "never traced" values in every plane."""
    mask = np.ones((h, w), bool)
    mask[np.ix_(traced_rows(h), traced_cols(w))] = False
    assert mask[0].all() and mask.sum() == w * h - len(traced_rows(h)) * len(traced_cols(w)), f"{what}: {int(mask.sum())} untraced pixels"
    for n, a in planes.items():
        value = MISS[n] if n in MISS else VIS_NEVER_TRACED[n]
        want = np.full((int(mask.sum()),) + a.shape[2:], value, a.dtype)
        assert same(a[mask], want), f"{what}: plane {n} of the pixels the reference never traces is not all {value!r}"


# ------------------------------------------------------------------ engine.rs:16-103, on [..., 3] arrays
def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]                     # engine.rs:85-87


def length(a):
    return np.sqrt(a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1] + a[..., 2] * a[..., 2])              # engine.rs:89-91


def cross(a, b):                                                                                       # engine.rs:93-99
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], -(a[..., 0] * b[..., 2] - a[..., 2] * b[..., 0]), a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def normalised(a):
    return a / length(a)[..., None]                                                                    # engine.rs:101-103


def as_usize(x):
    """Rust's `f64 as usize`: truncating, saturating, NaN and negatives -> 0."""
    x = np.asarray(x, np.float64)
    out = np.zeros(x.shape, np.uint64)
    big = x >= 18446744073709551616.0
    ok = (x > 0.0) & ~big
    out[ok] = x[ok].astype(np.uint64)
    out[big] = np.uint64(0xFFFFFFFFFFFFFFFF)
    return out


def light_vec(l):
    return np.array([l.v.x, l.v.y, l.v.z], np.float64)


# ------------------------------------------------------------------ the expected planes
def expected_planes(osc, A, lights, eye, dirs, surface_offset=1e-4):
    """The planes of the rays (eye, dirs[..., 3]) in the scene of the arrays dict A (pos, uv, nrm, mat, materials, textures) with `lights` (objects with
    kind, v.x, v.y, v.z): hit, t, u, v, tri, point, normal, material, lights in the shape of dirs[..., 0] (point, normal: of dirs), plus `bumped` (bool: the
    hit's normal went through a bump map).  osc is the oracle scene of the same arrays and lights; surface_offset is the option both were given."""
    shape = dirs.shape[:-1]
    D = np.ascontiguousarray(dirs, np.float64).reshape(-1, 3)
    N = len(D)
    eye = np.asarray(eye, np.float64)
    ans = list(POOL.map(lambda x: osc.intersect(eye, x), D))
    hit = np.array([a[0] for a in ans], bool)
    t = np.array([a[1] for a in ans], np.float64); u = np.array([a[2] for a in ans], np.float64); v = np.array([a[3] for a in ans], np.float64)
    tri = np.array([a[4] for a in ans], np.uint32)
    point = np.zeros((N, 3)); normal = np.zeros((N, 3)); material = np.full(N, NO_MATERIAL, np.uint32); mask = np.zeros(N, np.uint32); bumped = np.zeros(N, bool)
    h = np.flatnonzero(hit)
    if len(h):
        uv, nrm, mats = np.asarray(A["uv"], np.float64).reshape(-1, 3, 3), np.asarray(A["nrm"], np.float64).reshape(-1, 3, 3), np.asarray(A["mat"], np.uint32)
        T, U, V, K = t[h], u[h], v[h], tri[h]
        P = eye + D[h] * T[:, None]                                                                    # raytracer.rs:39
        M = mats[K]
        W = 1.0 - U - V                                                                                # raytracer.rs:43
        tex_x = uv[K, 1, 0] * U + uv[K, 2, 0] * V + uv[K, 0, 0] * W                                    # raytracer.rs:45-47
        tex_y = uv[K, 1, 1] * U + uv[K, 2, 1] * V + uv[K, 0, 1] * W                                    # raytracer.rs:48-50
        Nn = (nrm[K, 1] * U[:, None] + nrm[K, 2] * V[:, None]) + nrm[K, 0] * W[:, None]                # raytracer.rs:122-124
        B = np.zeros(len(h), bool)
        for m in np.unique(M):
            sel = np.flatnonzero(M == m)
            desc = A["materials"][int(m)]
            tex = np.asarray(A["textures"][desc["tex"]])
            th, tw = tex.shape[:2]
            xi = as_usize(tex_x[sel] * float(tw)) % np.uint64(tw)                                      # raytracer.rs:52
            yi = as_usize(tex_y[sel] * float(th)) % np.uint64(th)                                      # raytracer.rs:53
            if desc.get("bump", -1) < 0:
                continue
            bump = np.asarray(A["textures"][desc["bump"]])
            index = np.uint64(bump.shape[1]) * yi + xi                                                 # raytracer.rs:127-128: the colour texture's indices, the bump map's width
            bv = bump.reshape(-1, 3)[index.astype(np.int64)].astype(np.float64)
            bv = normalised(bv)
            bv = bv * 2.0 - np.array([1.0, 1.0, 1.0])                                                  # raytracer.rs:130-135
            n = Nn[sel]
            tg = cross(n, np.broadcast_to(np.array([0.0, 1.0, 0.0]), n.shape))                         # raytracer.rs:137-141
            zero = length(tg) == 0.0
            if zero.any():
                tg[zero] = cross(n[zero], np.broadcast_to(np.array([0.0, 0.0, 1.0]), n[zero].shape))  # raytracer.rs:143-149
            tg = normalised(tg)                                                                        # raytracer.rs:151
            bt = normalised(cross(n, tg))                                                              # raytracer.rs:152
            Nn[sel] = np.stack([dot(bv, tg), dot(bv, bt), dot(bv, n)], -1)                             # raytracer.rs:154-158
            B[sel] = True
        with np.errstate(invalid="ignore", divide="ignore"):
            Nn = normalised(Nn)                                                                        # raytracer.rs:161
        lit = np.zeros(len(h), np.uint32)
        for k, l in enumerate(lights):
            if l.kind != 1:
                lit |= np.uint32(1 << k)
                continue
            Ld = light_vec(l) - P                                                                      # raytracer.rs:170-179
            O = P + Nn * surface_offset
            Lm = length(Ld)
            occluded = np.fromiter(POOL.map(lambda i: osc.intersect(O[i], Ld[i], Lm[i])[0], range(len(h))), bool, len(h))
            lit |= np.where(occluded, 0, 1 << k).astype(np.uint32)
        point[h] = P; normal[h] = Nn; material[h] = M; mask[h] = lit; bumped[h] = B
    out = dict(hit=hit.astype(np.uint8).reshape(shape), t=t.reshape(shape), u=u.reshape(shape), v=v.reshape(shape), tri=tri.reshape(shape),
               point=point.reshape(shape + (3,)), normal=normal.reshape(shape + (3,)), material=material.reshape(shape), lights=mask.reshape(shape),
               bumped=bumped.reshape(shape))
    for a in out.values():
        a.setflags(write=False)
    return out


EXPECTED = ("hit", "point", "normal", "material", "lights")     # what the tests compare of expected_planes with surface(..., visibility=("hit",))


def lights_added_up(mask):
    """ctz(~mask): the reference's light loop adds up the lights [0, that) -- it ends at the first occluded point light (raytracer.rs:235-237)."""
    m = ~np.asarray(mask, np.uint32)
    low = m & (~m + np.uint32(1))                                # the lowest set bit
    return np.log2(low.astype(np.float64)).astype(np.int64)     # (bit 16 and above are always set in ~mask: low is never 0)


def shade(A, lights, dirs, planes, albedo):
    """compute_lighting_intensity and the colour of a non-mirror hit (raytracer.rs:192-304, 67-71, 104-108) from the planes point, normal, material, lights
    and the albedo plane; 0xFFFFFF where material says "miss".  dirs: the rays' directions.  Packed 0x00RRGGBB in the shape of planes["material"]."""
    shape = planes["material"].shape
    P, Nn = planes["point"].reshape(-1, 3), planes["normal"].reshape(-1, 3)
    M, mask, col = planes["material"].reshape(-1), planes["lights"].reshape(-1), np.asarray(albedo).reshape(-1)
    Vd = -np.ascontiguousarray(dirs, np.float64).reshape(-1, 3)
    n_eval = lights_added_up(mask)
    out = np.full(len(M), 0xFFFFFF, np.uint32)
    for m in np.unique(M[M != NO_MATERIAL]):
        sel = np.flatnonzero(M == m)
        desc = A["materials"][int(m)]
        ka, kd, ks = (np.array(desc[k], np.float64) for k in ("ka", "kd", "ks"))
        ns = float(desc["ns"])
        p, n, vv, ne = P[sel], Nn[sel], Vd[sel], n_eval[sel]
        I = np.zeros((len(sel), 3))
        for k, l in enumerate(lights):
            on = (k < ne)[:, None]
            if l.kind == 0:
                I = np.where(on, I + ka * float(l.intensity), I)                                      # raytracer.rs:207-209
                continue
            L = np.broadcast_to(light_vec(l), p.shape) if l.kind == 2 else light_vec(l) - p
            n_dot_l = dot(n, L)
            with np.errstate(invalid="ignore", divide="ignore"):
                diff = np.where((n_dot_l > 0.0)[:, None], ((kd * float(l.intensity)) * n_dot_l[:, None]) / (length(n) * length(L))[:, None], 0.0)   # raytracer.rs:260-277
                spec = np.zeros_like(I)
                if ns != -1.0:                                                                         # raytracer.rs:279-304
                    r = (n * 2.0) * dot(n, L)[:, None] - L
                    r_dot_v = dot(r, vv)
                    spec = np.where((r_dot_v > 0.0)[:, None], (ks * float(l.intensity)) * np.power(r_dot_v / (length(r) * length(vv)), ns)[:, None], 0.0)
            I = np.where(on, (I + diff) + spec, I)
        c = col[sel]
        local = np.stack([((c >> 16) & 255).astype(np.float64) * I[:, 0], ((c >> 8) & 255).astype(np.float64) * I[:, 1], (c & 255).astype(np.float64) * I[:, 2]], -1)
        q = np.where(local > 0.0, np.minimum(local, 255.0), 0.0).astype(np.uint32)                    # clamp(0.0, 255.0) as u8
        out[sel] = (q[:, 0] << 16) | (q[:, 1] << 8) | q[:, 2]
    return out.reshape(shape)
