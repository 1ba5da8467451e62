"""The specular skip (csrc/specular_skip.hpp, render.hip: specular_term) on the GPU: a specular term that the f64 lighting sum certainly absorbs is not
evaluated, and nothing that reaches a pixel may change.  RRT_FLAG_NO_SPECULAR_SKIP (specular_skip=False) evaluates every term, as before the skip existed.

  (a) One lit quad: two triangles with flat normals in the plane y = 0, one material, a 2x2 texture of value 255, an Ambient light of intensity 1 and one
      Point light.  4 096 rays from the eye, placed so that the cosine q between the mirrored light direction and the view direction sweeps -0.1 ... 1
      (half of them evenly, half evenly inside [0.78, 0.90], where terms with ns = 240 die out).  kd = 0, so the running sum I is ka * ambient alone.
      ns x ks x ka*ambient x sign of the intensity, every combination: colours with the flag equal colours without it bit for bit, in the default and in every
      forced walk, and both are within COLOUR_TOL of the oracle's get_ray_colour.
  (b) Teeth against a fixed threshold: with ka*ambient = 1e-30, ks*intensity = 1e20, ns = 240, the rays with 0.822 <= q < 0.843 carry a term far above I
      that a constant rule "q < 0.843: drop" would paint black.  Asserted from the oracle alone: at least 200 rays with q < 0.843 have a channel >= 100.
  (c) Frames: the teapot at 160x120 and 97x61, default lights and the default list reversed (tests/test_gpu_lighting.py's "default_reversed": Directional
      first): with and without the flag bit-identical in all modes; the no-cull frame within COLOUR_TOL of the oracle's; the same identity through the shade
      kernel and the per-ray shade kernel on a 64x48 region.
"""
import numpy as np
import pytest

from bitwise import assert_same_bits
from conftest import channels
from gpu_checks import ALL_MODES, N_THREADS, ORIGIN, ROOT_BOX, assert_frame_close, oracle_for, quad, flat_normals, row_dirs
from scenes import teapot_arrays_with_root as teapot_arrays  # noqa: F401  (fixtures: teapot_arrays)
from shade_checks import assert_shade_is_render
from shade_rays_checks import oracle_colours

pytestmark = pytest.mark.gpu

NS = (0.5, 1.0, 2.0, 10.0, 240.0, 500.0, 1e4, 1e6, -1.0, -3.0)
KS = (0.0, 1e-300, 1.0, 1e6, 1e20)
KA = (0.0, 1e-300, 1e-30, 1e-3, 1.0)
LIGHT = (0.0, 3.0, 6.0)
N_RAYS = 4096


def _quad_arrays():
    tris = quad((-3.0, 0.0, -5.0), (3.0, 0.0, -5.0), (3.0, 0.0, 9.0), (-3.0, 0.0, 9.0))
    pos = np.asarray(tris, np.float64)
    uv = np.zeros_like(pos); uv[..., 0] = pos[..., 0] * 0.1 + 0.5; uv[..., 1] = pos[..., 2] * 0.05 + 0.5
    return dict(pos=pos, uv=uv, nrm=flat_normals(tris, (0.0, 5.0, 0.0)), mat=np.zeros(2, np.uint32), materials=[_material(1.0, 1.0, 240.0)],
                textures=[np.full((2, 2, 3), 255, np.uint8)], root=ROOT_BOX)


def _material(ka, ks, ns):
    return dict(ka=(ka,) * 3, kd=(0.0, 0.0, 0.0), ks=(ks,) * 3, ns=ns, kr=0.0, tex=0, bump=-1)


def _cosine(p):
    """q = r.v / (|r| |v|) at the points p of the plane y = 0 (normal +y), seen from ORIGIN and lit from LIGHT (raytracer.rs:279-295)."""
    l = np.asarray(LIGHT) - p; v = np.asarray(ORIGIN) - p
    r = np.stack([-l[:, 0], l[:, 1], -l[:, 2]], 1)                 # 2 n (n.l) - l with n = (0, 1, 0)
    return (r * v).sum(1) / (np.linalg.norm(r, axis=1) * np.linalg.norm(v, axis=1))


def _quad_rays():
    """Directions from ORIGIN to N_RAYS points of the quad chosen by their q, and those q."""
    xs = np.linspace(-2.0, 2.0, 9); zs = np.linspace(-3.6, 7.0, 20001)      # q = 1 at (0, 0, -3.6), q = 0 near z = 6.4
    p = np.stack([np.repeat(xs, len(zs)), np.zeros(len(xs) * len(zs)), np.tile(zs, len(xs))], 1)
    q = _cosine(p)
    order = np.argsort(q)
    want = np.concatenate([np.linspace(-0.1, 1.0, N_RAYS // 2), np.linspace(0.78, 0.90, N_RAYS // 2)])
    pick = order[np.clip(np.searchsorted(q[order], want), 0, len(q) - 1)]
    return p[pick] - np.asarray(ORIGIN), q[pick]


@pytest.fixture(scope="module")
def quad_rig(rrt):
    """The quad scene, its rays, and one raytracer per (walk, flag): materials and lights are set per case (rrt_raytracer_set_materials / _set_lights)."""
    A = _quad_arrays()
    sd = rrt.SceneData.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], A["materials"], A["textures"])
    D, q = _quad_rays()
    O = np.tile(ORIGIN, (len(D), 1))
    lights = [rrt.Light.Ambient(1.0), rrt.Light.Point(1.0, rrt.Vector3d(*LIGHT))]
    rts = {(mode, skip): rrt.RayTracer(sd, lights, box_filter=mode, specular_skip=skip) for mode in ALL_MODES for skip in (True, False)}
    assert (q > 0.99).any() and (q < 0.0).any() and ((q > 0.822) & (q < 0.843)).sum() >= 300
    assert rts[(None, True)].intersect_rays(O, D)[0].all(), "a ray misses the quad"
    return A, O, D, q, rts


@pytest.mark.parametrize("sign", (1.0, -1.0))
@pytest.mark.parametrize("ns", NS)
def test_lit_quad(rrt, ob, quad_rig, ns, sign):
    A, O, D, q, rts = quad_rig
    lights = [rrt.Light.Ambient(1.0), rrt.Light.Point(sign, rrt.Vector3d(*LIGHT))]
    for ks in KS:
        for ka in KA:
            what = f"quad ns={ns:g} ks={ks:g} ka*ambient={ka:g} intensity={sign:g}"
            mats = [_material(ka, ks, ns)]
            ref = oracle_colours(oracle_for(ob, dict(A, materials=mats), lights), O, D)
            for rt in rts.values():
                rt.set_lights(lights); rt.set_materials(mats)
            for mode in ALL_MODES:
                full = rts[(mode, False)].get_ray_colours(O, D)
                got = rts[(mode, True)].get_ray_colours(O, D)
                n = int((got != full).sum())
                assert n == 0, f"{what}, walk {mode}: {n} of {len(D)} ray colours change with the skip"
                assert_frame_close(full, ref, f"{what}, walk {mode}: every term evaluated vs the oracle")
            if ns == 240.0 and sign == 1.0 and ks == 1e20 and ka == 1e-30:                                      # (b)
                teeth = int(((q < 0.843) & (channels(ref).max(-1) >= 100)).sum())
                print(f"\n[specular skip] {what}: {teeth} rays with q < 0.843 and a channel >= 100")
                assert teeth >= 200, f"{what}: only {teeth} rays separate the exact rule from a fixed threshold q < 0.843 (< 200)"


# ------------------------------------------------------------------ (c) frames
SIZES = ((160, 120), (97, 61))
REGION = (48, 36, 64, 48)            # of the 160x120 frame: the teapot's body


@pytest.mark.parametrize("which", ("default", "default_reversed"))
def test_teapot_frames(rrt, ob, teapot, teapot_arrays, which):
    lights = rrt.default_lights() if which == "default" else rrt.default_lights()[::-1]
    assert which == "default" or lights[0].kind == 2
    osc = oracle_for(ob, teapot_arrays, lights)
    exact = {skip: rrt.RayTracer(teapot, lights, no_cull=True, specular_skip=skip) for skip in (True, False)}
    rts = {(mode, skip): rrt.RayTracer(teapot, lights, box_filter=mode, specular_skip=skip) for mode in ALL_MODES for skip in (True, False)}
    for w, h in SIZES:
        ref = exact[False].render(w, h)
        assert_frame_close(ref, osc.render(w, h, n_threads=N_THREADS)[0], f"teapot {which} {w}x{h}: no-cull frame vs the oracle")
        assert_same_bits(exact[True].render(w, h), ref, f"teapot {which} {w}x{h}, no-cull: with the skip vs without")
        for (mode, skip), rt in rts.items():
            assert_same_bits(rt.render(w, h), ref, f"teapot {which} {w}x{h}, walk {mode}, skip {skip}: vs the no-cull frame")
    # the shade kernel and the per-ray shade kernel, on a region
    w, h = SIZES[0]
    x0, y0, rw, rh = REGION
    d = np.stack([row_dirs(w, h, r, np.arange(x0, x0 + rw)) for r in range(y0, y0 + rh)]).reshape(-1, 3)
    o = np.tile(ORIGIN, (len(d), 1))
    for mode in ALL_MODES:
        frames = {}
        for skip in (True, False):
            rt = rts[(mode, skip)]
            frames[skip], _ = assert_shade_is_render(rt, w, h, f"teapot {which}, walk {mode}, skip {skip}", region=REGION)
            colours = rt.get_ray_colours(o, d)
            shaded = rt.shade_rays(d, rt.surface_rays(o, d))["colour"]
            n = int((shaded != colours).sum())
            assert n == 0, f"teapot {which}, walk {mode}, skip {skip}: {n} of {len(d)} colours of shade_rays differ from get_ray_colours"
            frames[skip] = (frames[skip], colours)
        assert_same_bits(frames[True][0], frames[False][0], f"teapot {which}, walk {mode}: frame with the skip vs without")
        n = int((frames[True][1] != frames[False][1]).sum())
        assert n == 0, f"teapot {which}, walk {mode}: {n} of {len(d)} ray colours change with the skip"
