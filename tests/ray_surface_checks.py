"""Helpers of the tests of the per-ray surface query (include/rrt.h: rrt_surface_rays): the expected arrays of arbitrary rays, restated on the host from the
reference around the oracle's intersector, the reference's reflection recursion followed level by level from those arrays, and the record's arrays as device
tensors filled with sentinels (device_arrays, to_host).

Plain module, not a test module: pytest does not rewrite its asserts, so every assert here states both values in its message.  It holds no fixtures.

expected_ray_planes restates surface_checks.expected_planes for rays that each have an origin and a bound of their own, and adds what the per-ray call adds:
    raytracer.rs:52-55    the colour texel (albedo)
    raytracer.rs:78-82    the reflection ray: origin = point + normal * surface_offset, direction = normalised(d - (normal * 2.0) * dot(d, normal))
One rounded f64 operation per reference operation, with surface_checks' dot / length / cross / normalised (no np.dot, np.cross, np.linalg.norm).
"""
import numpy as np

from bitwise import bits
from conftest import channels
from gpu_checks import POOL
from surface_checks import NO_MATERIAL, as_usize, cross, dot, length, light_vec, lights_added_up, normalised, shade

NAMES = ("hit", "t", "u", "v", "tri", "albedo", "point", "normal", "material", "lights", "next_origin", "next_dir")   # rrt_ray_surface, in its order
VECTORS = ("point", "normal", "next_origin", "next_dir")
WHITE = 0x00FFFFFF
RAY_MISS = dict(hit=0, t=0.0, u=0.0, v=0.0, tri=0xFFFFFFFF, albedo=WHITE, point=0.0, normal=0.0, material=NO_MATERIAL, lights=0, next_origin=0.0, next_dir=0.0)
DTYPES = dict(hit=np.uint8, t=np.float64, u=np.float64, v=np.float64, tri=np.uint32, albedo=np.uint32, point=np.float64, normal=np.float64, material=np.uint32,
              lights=np.uint32, next_origin=np.float64, next_dir=np.float64)
SENTINEL = dict(hit=0xA5, t=-12345.5, u=-12345.5, v=-12345.5, tri=-1515870811, albedo=-1515870811, point=-12345.5, normal=-12345.5, material=-1515870811,
                lights=-1515870811, next_origin=-12345.5, next_dir=-12345.5)                 # what device_arrays fills an output with (0xA5A5A5A5 as int32)


def reflected(D, Nn):
    """raytracer.rs:78-79: normalised(d - (n * 2.0) * dot(d, n))"""
    d_dot_n = dot(D, Nn)
    with np.errstate(invalid="ignore", divide="ignore"):
        return normalised(D - (Nn * 2.0) * d_dot_n[..., None])


def expected_ray_planes(osc, A, lights, O, D, M=None, surface_offset=1e-4):
    """The twelve arrays of rrt_surface_rays for the rays (O[i], D[i]) with the bounds M[i] (None: +inf) in the scene of the arrays dict A with `lights` (objects
    with kind, v.x, v.y, v.z), in the leading shape of D, plus `bumped` (bool: the hit's normal went through a bump map).  osc is the oracle scene of the same
    arrays and lights; surface_offset is the option both were given.  O may be one point for all rays."""
    D = np.asarray(D, np.float64)
    shape = D.shape[:-1]
    D = np.ascontiguousarray(D).reshape(-1, 3)
    N = len(D)
    O = np.ascontiguousarray(np.broadcast_to(np.asarray(O, np.float64).reshape(-1, 3), (N, 3)))
    M = np.full(N, np.inf) if M is None else np.ascontiguousarray(np.broadcast_to(np.asarray(M, np.float64).reshape(-1), (N,)))
    ans = list(POOL.map(lambda i: osc.intersect(O[i], D[i], M[i]), range(N)))
    hit = np.array([a[0] for a in ans], bool)
    t = np.array([a[1] for a in ans], np.float64); u = np.array([a[2] for a in ans], np.float64); v = np.array([a[3] for a in ans], np.float64)
    tri = np.array([a[4] for a in ans], np.uint32)
    point = np.zeros((N, 3)); normal = np.zeros((N, 3)); nxt_o = np.zeros((N, 3)); nxt_d = np.zeros((N, 3))
    material = np.full(N, NO_MATERIAL, np.uint32); mask = np.zeros(N, np.uint32); albedo = np.full(N, WHITE, np.uint32); bumped = np.zeros(N, bool)
    h = np.flatnonzero(hit)
    if len(h):
        uv, nrm, mats = np.asarray(A["uv"], np.float64).reshape(-1, 3, 3), np.asarray(A["nrm"], np.float64).reshape(-1, 3, 3), np.asarray(A["mat"], np.uint32)
        T, U, V, K = t[h], u[h], v[h], tri[h]
        P = O[h] + D[h] * T[:, None]                                                                   # raytracer.rs:39
        Mt = mats[K]
        W = 1.0 - U - V                                                                                # raytracer.rs:43
        tex_x = uv[K, 1, 0] * U + uv[K, 2, 0] * V + uv[K, 0, 0] * W                                    # raytracer.rs:45-47
        tex_y = uv[K, 1, 1] * U + uv[K, 2, 1] * V + uv[K, 0, 1] * W                                    # raytracer.rs:48-50
        Nn = (nrm[K, 1] * U[:, None] + nrm[K, 2] * V[:, None]) + nrm[K, 0] * W[:, None]                # raytracer.rs:122-124
        B = np.zeros(len(h), bool)
        col = np.zeros(len(h), np.uint32)
        for m in np.unique(Mt):
            sel = np.flatnonzero(Mt == m)
            desc = A["materials"][int(m)]
            tex = np.asarray(A["textures"][desc["tex"]])
            th, tw = tex.shape[:2]
            xi = as_usize(tex_x[sel] * float(tw)) % np.uint64(tw)                                      # raytracer.rs:52
            yi = as_usize(tex_y[sel] * float(th)) % np.uint64(th)                                      # raytracer.rs:53
            texel = tex.reshape(-1, 3)[(np.uint64(tw) * yi + xi).astype(np.int64)].astype(np.uint32)   # raytracer.rs:55
            col[sel] = (texel[:, 0] << 16) | (texel[:, 1] << 8) | texel[:, 2]
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
        Onext = P + Nn * surface_offset                                                                # raytracer.rs:82, :170
        lit = np.zeros(len(h), np.uint32)
        for k, l in enumerate(lights):
            if l.kind != 1:
                lit |= np.uint32(1 << k)
                continue
            Ld = light_vec(l) - P                                                                      # raytracer.rs:170-179
            Lm = length(Ld)
            occluded = np.fromiter(POOL.map(lambda i: osc.intersect(Onext[i], Ld[i], Lm[i])[0], range(len(h))), bool, len(h))
            lit |= np.where(occluded, 0, 1 << k).astype(np.uint32)
        point[h] = P; normal[h] = Nn; material[h] = Mt; mask[h] = lit; bumped[h] = B; albedo[h] = col
        nxt_o[h] = Onext; nxt_d[h] = reflected(D[h], Nn)
    out = dict(hit=hit.astype(np.uint8).reshape(shape), t=t.reshape(shape), u=u.reshape(shape), v=v.reshape(shape), tri=tri.reshape(shape),
               albedo=albedo.reshape(shape), point=point.reshape(shape + (3,)), normal=normal.reshape(shape + (3,)), material=material.reshape(shape),
               lights=mask.reshape(shape), next_origin=nxt_o.reshape(shape + (3,)), next_dir=nxt_d.reshape(shape + (3,)), bumped=bumped.reshape(shape))
    for a in out.values():
        a.setflags(write=False)
    return out


def assert_miss_values(got, sel, what):
    """The rays `sel` (bool or indices) carry the miss values in every array of `got`."""
    for n, a in got.items():
        part = np.asarray(a)[sel]
        want = np.full(part.shape, RAY_MISS[n], DTYPES[n])
        assert part.dtype == want.dtype and (bits(part) == bits(want)).all(), f"{what}: array {n} of a miss is not all {RAY_MISS[n]!r}"


def rows(planes, sel):
    return {n: np.asarray(a)[sel] for n, a in planes.items()}


# ------------------------------------------------------------------ the reference's recursion from the arrays
def kr_table(A):
    """kr per material index, and 0.0 for anything at or beyond the table (0xFFFFFFFF: a miss)."""
    return np.array([float(m["kr"]) for m in A["materials"]] + [0.0])


def kr_of(A, material):
    tab = kr_table(A)
    return tab[np.minimum(np.asarray(material, np.int64), len(tab) - 1)]


def clamp_u8(x):
    """clamp(0.0, 255.0) as u8, raytracer.rs:97-108"""
    return np.where(x > 0.0, np.minimum(x, 255.0), 0.0).astype(np.uint32)


def pack(q):
    return ((q[..., 0] << 16) | (q[..., 1] << 8) | q[..., 2]).astype(np.uint32)


def local_colour(A, lights, dirs, planes):
    """The f64 `local` colour of raytracer.rs:67-71 per ray -- albedo channel times compute_lighting_intensity (raytracer.rs:192-304) -- which the reference keeps
    UNquantised while it mixes in the reflection (raytracer.rs:89-95).  surface_checks.shade returns this value clamped and truncated; follow_chain asserts
    that on every level, so this is shade's arithmetic, not a second opinion.  Rows of a miss are 0."""
    P, Nn = planes["point"].reshape(-1, 3), planes["normal"].reshape(-1, 3)
    Mi, mask, col = planes["material"].reshape(-1), planes["lights"].reshape(-1), np.asarray(planes["albedo"]).reshape(-1)
    Vd = -np.ascontiguousarray(dirs, np.float64).reshape(-1, 3)
    n_eval = lights_added_up(mask)
    out = np.zeros((len(Mi), 3))
    for m in np.unique(Mi[Mi != NO_MATERIAL]):
        sel = np.flatnonzero(Mi == m)
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
        out[sel] = np.stack([((c >> 16) & 255).astype(np.float64) * I[:, 0], ((c >> 8) & 255).astype(np.float64) * I[:, 1], (c & 255).astype(np.float64) * I[:, 2]], -1)
    return out


class HostChain:
    """Feeds follow_chain from RayTracer.surface_rays: the rays of a level are numpy arrays."""
    def __init__(self, rt, O, D):
        self.rt, self.o, self.d, self.m = rt, np.ascontiguousarray(O, np.float64).reshape(-1, 3), np.ascontiguousarray(D, np.float64).reshape(-1, 3), None
        self.calls = 0

    def level(self):
        """(the level's directions, its twelve arrays) on the host"""
        self.calls += 1
        self.planes = self.rt.surface_rays(self.o, self.d, self.m)
        return self.d, self.planes

    def descend(self, go, compact):
        if compact:
            self.o, self.d, self.m = self.planes["next_origin"][go], self.planes["next_dir"][go], None
        else:
            self.o, self.d, self.m = self.planes["next_origin"], self.planes["next_dir"], np.where(go, np.inf, 0.0)


def follow_chain(chain, A, lights, max_depth=5, compact=True):
    """get_ray_colour_recursive (raytracer.rs:29-112) from the arrays of the per-ray call, level by level: chain.level() gives a level's directions and arrays,
    chain.descend(go, compact) makes the next level of the rays `go` -- hits on a material with kr > 0 below the depth limit (raytracer.rs:76) -- from their
    next_origin / next_dir: compact = only those rays; otherwise the whole batch again, with max_t = 0.0 for the dead ones.  A level is shaded on the host
    with surface_checks.shade; the unwind is local * (1 - kr) + reflected_u8 * kr, clamped and truncated at every level (raytracer.rs:89-101).
    Returns (packed colours of the first level's rays, rays alive per level)."""
    levels, alive = [], []
    sel = None                                                   # not compact: the rays of the batch that are alive at this level
    for depth in range(max_depth + 1):
        dirs, pl = chain.level()
        hit = pl["hit"].astype(bool)
        if sel is not None:
            assert not hit[~sel].any(), f"level {depth}: a ray with max_t = 0.0 reports a hit"
            assert_miss_values({n: pl[n] for n in NAMES}, ~sel, f"level {depth}, dead rays")
        with np.errstate(invalid="ignore", divide="ignore"):
            u8 = shade(A, lights, dirs, pl, pl["albedo"])
            local = local_colour(A, lights, dirs, pl)
        same = pack(clamp_u8(local))[hit] == u8[hit]
        assert same.all(), f"level {depth}: local_colour, clamped and truncated, is not surface_checks.shade on {int((~same).sum())} of {int(hit.sum())} hits"
        kr = kr_of(A, pl["material"])
        go = hit & (kr > 0.0) & (depth < max_depth)              # raytracer.rs:76
        levels.append((go, local, kr, u8))
        alive.append(int(len(hit) if sel is None else sel.sum()))
        if not go.any():
            break
        chain.descend(go, compact)
        sel = None if compact else go
    c = levels[-1][3]
    for go, local, kr, u8 in reversed(levels[:-1]):
        below = channels(c if compact else c[go]).astype(np.float64)
        mixed = local[go] * (1.0 - kr[go])[:, None] + below * kr[go][:, None]                          # raytracer.rs:89-95
        out = u8.copy()
        out[go] = pack(clamp_u8(mixed))                                                                # raytracer.rs:97-101
        c = out
    return c, alive


# ------------------------------------------------------------------ the arrays on the device (torch is the caller's: this module imports none)
def device_arrays(torch, n, names=NAMES):
    """{name: flat device tensor for n rays, filled with SENTINEL[name]}"""
    kinds = {np.uint8: torch.uint8, np.float64: torch.float64, np.uint32: torch.int32}
    return {name: torch.full((n * (3 if name in VECTORS else 1),), SENTINEL[name], dtype=kinds[DTYPES[name]], device="cuda") for name in names}


def to_host(tensors, n):
    return {name: t.cpu().numpy().view(DTYPES[name]).reshape((n, 3) if name in VECTORS else (n,)) for name, t in tensors.items()}
