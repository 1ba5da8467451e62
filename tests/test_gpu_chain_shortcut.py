"""The chain shortcut of the bundle-filter walk (render.hip: chain_target; device_scene.hpp: DevChain) against the CPU oracle.

A CHAIN NODE is an internal node with exactly one child whose triangle_count > 0; a chain is a maximal run of chain nodes below some parent, down to
its END, the first node on the path that is no chain node.  The reference's tree has such runs wherever a scene is small against the root box
(octree.rs:77-80: the first triangle that reaches a node stays in it).  A lane whose ray certainly crosses the END's subtree box (fp32 test of the box
shrunk by twice the index pad) and misses the padded boxes of the chain nodes' own triangles enters the END directly.  Every case below

  * is compared bit for bit with oracle.intersect (hit, triangle, t, u, v) through rrt_intersect_rays, and with the oracle's frame where colour is
    involved, in the three forced walk variants, with the shortcut on and off (RRT_FLAG_NO_CHAIN_SHORTCUT);
  * first proves on the CPU -- from the oracle's octree and a brute-force Moller-Trumbore in numpy -- that the situation it names is present in its
    rays (`_situations`, also run as a CPU test of its own), and that the scene has the chains it is meant to have (`n_chains`).

The hand-built scene (`_scene`): root +-20; triangle 0 stays in the root; C1 stays in d1 = [0,20]^3, C2 in d2 = [0,10]^3; everything else lies in
D = [0,5]^3, which has several non-empty children.  C1 lies in front of D's triangles (inside D's subtree box), C2 outside D's subtree box; TIE is
coplanar with C1 (dyadic coordinates and axis-parallel rays: the two t are the same bits); GRAZE ends 2^-20 short of the face x = 5 of D's octant box
(a child only takes a triangle that lies strictly inside it, so no triangle of D's subtree touches D's faces), and rays run in, just inside and just
outside the faces x = 0, 5 and 10 of the octant boxes.  A build that redirects without the triangle-box condition loses C1 (case 1) and, for the rays
that cross an empty corner of D's box before they reach C2, C2 (cases 2 and 4).  A build that redirects on the UNSHRUNK box fails nothing here and cannot:
a ray that misses an octant box but passes the padded subtree box inside it cannot hit a triangle of that subtree, since none reaches the octant's faces;
the shrink is the margin for the fp32 evaluation (profiles/r05_chain_shortcut.txt, section D).

model2.obj: the issue that introduced the shortcut expected n_chains == 4 and n_chain_nodes == 8.  Those are the chains BELOW THE ROOT (asserted
here).  By the definition above -- which is the one the issue states -- the oracle's octree of model2.obj has 63 chains, 24 of which hold at most
K = 4 own triangles (30 chain nodes); the test derives both figures from the oracle's octree and asserts them.
"""
import os

import numpy as np
import pytest

from conftest import ASSETS
from gpu_checks import (CHAIN_CAMERA as CAMERA, CHAIN_D_TRIS as D_TRIS, CHAIN_LIGHTS as LIGHTS, CHAIN_PAD as PAD, COLOUR_TOL, FORCED_MODES, N_THREADS,
                        ROOT_BOX, assert_frame_close, assert_rays_match_oracle, chain_main_rays as _main_rays, chain_rrt_lights as _rrt_lights,
                        chain_scene as _scene, chain_z_rays as _z_rays, checker, oracle_for)

EPS = 2.220446049250313e-16
K = 4                                                     # kChainMaxTris, device_scene.hpp
NAN, INF = float("nan"), float("inf")


# ------------------------------------------------------------------ chains of an octree, by the definition
def chains_of(tree):
    """Every maximal chain of the octree dict: (parent, [chain nodes], end, [own triangle indices of the chain nodes in chain order])."""
    fc, tc, off, idx = tree["first_child"], tree["tri_count"], tree["own_off"], tree["own_idx"]
    kids = lambda c: [int(fc[c]) + k for k in range(8) if tc[int(fc[c]) + k] > 0] if fc[c] else []
    is_chain = lambda c: len(kids(c)) == 1
    out = []
    for p in range(len(fc)):
        if not fc[p] or (p != 0 and is_chain(p)):
            continue
        for c in range(int(fc[p]), int(fc[p]) + 8):
            if not is_chain(c):
                continue
            nodes, d = [], c
            while is_chain(d):
                nodes.append(d); d = kids(d)[0]
            out.append((p, nodes, d, [int(t) for n in nodes for t in idx[off[n]:off[n + 1]]]))
    return out


def with_record(chains):
    return [c for c in chains if len(c[3]) <= K]


def subtree_tris(tree, node):
    fc, off, idx = tree["first_child"], tree["own_off"], tree["own_idx"]
    todo, tris = [node], []
    while todo:
        n = todo.pop(); tris += [int(t) for t in idx[off[n]:off[n + 1]]]
        if fc[n]: todo += list(range(int(fc[n]), int(fc[n]) + 8))
    return tris


def brute_force(pos, o, d):
    """Ray::intersect_with_triangle (ray.rs:56-94) against every triangle: t per triangle, NaN where the ray misses it."""
    v1, e1, e2 = pos[:, 0], pos[:, 1] - pos[:, 0], pos[:, 2] - pos[:, 0]
    h = np.cross(d, e2); a = (e1 * h).sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = 1.0 / a; s = o - v1; u = f * (s * h).sum(1); q = np.cross(s, e1); v = f * (q @ d); t = f * (e2 * q).sum(1)
        ok = ~((a > -EPS) & (a < EPS)) & (u >= 0.0) & (u <= 1.0) & (v >= 0.0) & (u + v <= 1.0) & (t > EPS)
    return np.where(ok, t, np.nan)


# ------------------------------------------------------------------ the hand-built scenes: gpu_checks.py (chain_scene, chain_main_rays)


def _edge_rays():
    """Case 7: NaN, infinite and zero directions and origins, among ordinary rays of the same waves."""
    O, D = _z_rays(np.arange(1.0625, 4.0, 0.25), np.arange(1.0625, 4.0, 0.25))
    O, D = O.copy(), D.copy()
    bad = [((2.75, 2.125, -5), (0, 0, 0)), ((2.75, 2.125, -5), (NAN, 0, 1)), ((2.75, 2.125, -5), (0, NAN, 1)), ((2.75, 2.125, -5), (0, 0, NAN)),
           ((2.75, 2.125, -5), (0, 0, INF)), ((2.75, 2.125, -5), (INF, 0, 1)), ((2.75, 2.125, -5), (0, -INF, 1)), ((NAN, 2.125, -5), (0, 0, 1)),
           ((2.75, INF, -5), (0, 0, 1)), ((2.75, 2.125, -INF), (0, 0, 1)), ((2.75, 2.125, -5), (0, 0, 1e-320)), ((2.75, 2.125, -5), (0, 0, 1e300)),
           ((2.75, 2.125, -1e6), (0, 0, 1)), ((7.25, 7.25, -5), (0, 0, 0)), ((7.25, 7.25, -5), (NAN, NAN, NAN))]
    for i, (o, d) in enumerate(bad):
        O[3 + 7 * i], D[3 + 7 * i] = o, d
    return O, D, np.full(len(O), INF)


def _situations(ob):
    """Builds the oracle scenes and rays of cases 1-7 and asserts that every named situation is present.  Returns what the GPU tests need."""
    out = {}
    A, names = _scene("main"); names = np.array(names)
    osc = oracle_for(ob, A, LIGHTS, CAMERA); tree = osc.octree(); ch = chains_of(tree)
    parent, nodes, end, ctris = ch[0]
    assert parent == 0 and len(nodes) == 2 and [names[t] for t in ctris] == ["c1", "c2"], ch
    below = subtree_tris(tree, end)
    assert sorted(names[below]) == sorted(D_TRIS), (sorted(names[below]), "the chain's end holds D's triangles")
    assert sum(tree["tri_count"][int(tree["first_child"][end]) + k] > 0 for k in range(8)) >= 2, "the end is no chain node"
    dlo, dhi = A["pos"][below].min((0, 1)), A["pos"][below].max((0, 1))                       # D's tight subtree box
    hl, hh = A["pos"][subtree_tris(tree, nodes[0])].min((0, 1)), A["pos"][subtree_tris(tree, nodes[0])].max((0, 1))
    R = _main_rays()
    idx = lambda n: int(np.flatnonzero(names == n)[0])
    n = dict(nearest_is_chain=0, chain_then_below=0, tie=0, tie_outer_wins=0, c2_outside_end=0, c2_through_end=0, band=0, graze=0, graze_hits=0, shadow_occluded=0, shadow_beyond=0)
    O, D, M = R["on_c1"]
    for o, d in zip(O, D):
        t = brute_force(A["pos"], o, d); ref = osc.intersect(o, d)
        if t[idx("c1")] == np.nanmin(t):
            n["nearest_is_chain"] += 1
            n["chain_then_below"] += bool(np.any(t[below] > t[idx("c1")]))
            if t[idx("tie")] == t[idx("c1")]:
                n["tie"] += 1; n["tie_outer_wins"] += ref[4] == idx("c1")
    O, D, M = R["on_c2"]
    for o, d in zip(O, D):
        t = brute_force(A["pos"], o, d)
        inside = np.all((o[:2] >= dlo[:2]) & (o[:2] <= dhi[:2])) if d[0] == 0 and d[1] == 0 else False
        n["c2_outside_end"] += bool(t[idx("c2")] == np.nanmin(t) and not inside and np.all(A["pos"][idx("c2")].min(0) > dhi))
    for o, d in zip(*R["through_end"][:2]):                                                      # C2 behind an empty corner of D's (shrunk) subtree box
        p_ = o + 3.0 * d; t = brute_force(A["pos"], o, d)
        n["c2_through_end"] += bool(np.all(p_ > dlo + 4.0 * PAD) and np.all(p_ < dhi - 4.0 * PAD) and t[idx("c2")] == np.nanmin(t) and np.isfinite(t).sum() == 1)
    O, D, M = R["band"]
    for o, d in zip(O, D):
        in_head = np.all((o[:2] >= hl[:2] - PAD) & (o[:2] <= hh[:2] + PAD))
        near_face = min(np.abs(o[:2] - dlo[:2]).min(), np.abs(o[:2] - dhi[:2]).min()) <= 2.0 * PAD
        n["band"] += bool(in_head and near_face)
        t = brute_force(A["pos"], o, d); ref = osc.intersect(o, d)
        n["graze"] += bool(min(abs(o[0] - f) for f in (0.0, 5.0, 10.0)) <= 2.0 ** -19)
        n["graze_hits"] += bool(np.isfinite(t[idx("graze")]) and ref[0] and ref[4] == idx("graze"))
    O, D, M = R["shadow"]
    for o, d, m in zip(O, D, M):
        t = brute_force(A["pos"], o, d); hit = osc.intersect(o, d, m)[0]
        assert np.isfinite(t[idx("c2")]) and np.nansum(np.isfinite(t)) == 1, "only C2 lies on a shadow ray"
        n["shadow_occluded"] += bool(hit and t[idx("c2")] < m); n["shadow_beyond"] += bool(not hit and t[idx("c2")] >= m)
    need = dict(nearest_is_chain=40, chain_then_below=40, tie=10, tie_outer_wins=10, c2_outside_end=30, c2_through_end=30, band=60, graze=100, graze_hits=10, shadow_occluded=40, shadow_beyond=40)
    for k, v in need.items():
        assert n[k] >= v, f"situation {k}: {n[k]} rays (< {v}); all: {n}"
    out["main"] = (A, osc, R, len(with_record(ch)), n)
    for which in ("leaf_end", "long_lists", "non_root_parent", "pokes_out"):
        A2, names2 = _scene(which); osc2 = oracle_for(ob, A2, LIGHTS, CAMERA); tree2 = osc2.octree(); ch2 = chains_of(tree2)
        p2, nodes2, end2, tris2 = ch2[0]                                       # the chain that the scene is about
        want_rec = len(with_record(ch2))
        assert (len(tris2) <= K) == (which != "long_lists"), f"{which}: chains {ch2}"
        if which == "leaf_end": assert tree2["first_child"][end2] == 0 and tree2["tri_count"][end2] == 1, "the chain ends in a non-empty leaf"
        if which == "long_lists": assert len(tris2) > K, f"{len(tris2)} own triangles in the chain (<= K)"
        if which == "non_root_parent": assert p2 != 0 and len(nodes2) == 2, ch2
        if which == "pokes_out": assert A2["pos"].max() > 20.0
        out[which] = (A2, osc2, want_rec if which != "pokes_out" else 0)
    return out


def test_switch_flag_matches_the_header(rrt):
    import re
    hdr = open(os.path.join(os.path.dirname(ASSETS), "include", "rrt.h")).read()
    m = re.search(r"#define RRT_FLAG_NO_CHAIN_SHORTCUT \(1u << (\d+)\)", hdr)
    assert m and (1 << int(m.group(1))) == rrt.FLAG_NO_CHAIN_SHORTCUT == 32
    taken = [int(v) for v in re.findall(r"#define RRT_FLAG_\w+ (\d+)u", hdr)]
    assert rrt.FLAG_NO_CHAIN_SHORTCUT not in taken and all(v & rrt.FLAG_NO_CHAIN_SHORTCUT == 0 for v in taken), taken


def test_chain_situations_hold_on_the_cpu(ob):
    s = _situations(ob)
    print(f"\n[chain shortcut] rays per situation: {s['main'][4]}")


# ------------------------------------------------------------------ GPU
def _raytracers(rrt, A, camera=CAMERA, **kw):
    """(label, raytracer) for the three forced walks, with the shortcut on and off."""
    sd = rrt.SceneData.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], A["materials"], A["textures"])
    for mode in FORCED_MODES:
        for on in (True, False):
            yield f"walk {mode}, shortcut {'on' if on else 'off'}", rrt.RayTracer(sd, _rrt_lights(rrt), rrt.Vector3d(*camera), box_filter=mode, chain_shortcut=on, **kw)


def _check_rays(rt, osc, O, D, M, what):
    assert_rays_match_oracle(rt.intersect_rays(O, D, M), osc, O, D, M, what)
    cols = rt.get_ray_colours(O, D)
    ref = np.fromiter((osc.get_ray_colour(O[i], D[i]) for i in range(len(O))), np.uint32, len(O))
    assert_frame_close(cols, ref, what + " (colours)")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["on_c1", "on_c2", "band", "shadow"], ids=["1_chain_triangle_is_hit", "2_chain_triangle_outside_end", "3_band_and_grazing", "4_shadow_queries"])
def test_hand_built_chain_matches_the_oracle(rrt, ob, case):
    A, osc, R, n_chains, _ = _situations(ob)["main"]
    O, D, M = R[case]
    for label, rt in _raytracers(rrt, A):
        assert rt.chain_info["n_chains"] == n_chains > 0, (label, rt.chain_info)
        _check_rays(rt, osc, O, D, M, f"case {case}, {label}")


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["leaf_end", "long_lists", "non_root_parent", "pokes_out"])
def test_other_chain_shapes_match_the_oracle(rrt, ob, which):
    """Cases 5 and 6: a chain that ends in a leaf, one with more than K own triangles (no record), one below a non-root parent, and a scene with a
    triangle poking out of the root (inner_shrink == 0: no shortcut)."""
    A, osc, n_rec = _situations(ob)[which]
    scale = 0.5 if which == "non_root_parent" else 1.0
    rays = _main_rays()
    O = np.concatenate([rays[k][0] for k in rays]) * [scale, scale, 1.0]; D = np.concatenate([rays[k][1] for k in rays]); M = np.concatenate([rays[k][2] for k in rays])
    for label, rt in _raytracers(rrt, A):
        assert rt.chain_info["n_chains"] == n_rec, (which, label, rt.chain_info)
        _check_rays(rt, osc, O, D, M, f"{which}, {label}")
        frame = rt.render(160, 120)
        assert_frame_close(frame, osc.render(160, 120, n_threads=N_THREADS)[0], f"{which}, {label}, frame")


@pytest.mark.gpu
def test_edge_rays_and_no_cull_are_never_redirected(rrt, ob):
    """Case 7."""
    A, osc, _, n_chains, _ = _situations(ob)["main"]
    O, D, M = _edge_rays()
    assert np.isnan(D).any() and np.isinf(D).any() and (D == 0).all(1).any() and np.isnan(O).any() and np.isinf(O).any()
    for label, rt in _raytracers(rrt, A):
        assert_rays_match_oracle(rt.intersect_rays(O, D, M), osc, O, D, M, f"edge rays, {label}")
    rays = _main_rays()
    O2 = np.concatenate([rays[k][0] for k in rays] + [O]); D2 = np.concatenate([rays[k][1] for k in rays] + [D]); M2 = np.concatenate([rays[k][2] for k in rays] + [M])
    for label, rt in _raytracers(rrt, A, no_cull=True):
        assert rt.chain_info == {"n_chains": 0, "n_chain_nodes": 0}, (label, rt.chain_info)
        assert_rays_match_oracle(rt.intersect_rays(O2, D2, M2), osc, O2, D2, M2, f"no_cull, {label}")


def _random_scene(seed):
    """1 .. 3000 small triangles inside [1, 4]^3 of the +-20 root (chains of two or three nodes below the root), mirror material."""
    rng = np.random.default_rng(1000 + seed)
    n = int(np.round(3000 ** rng.random()))
    p = rng.uniform(1.2, 3.8, (n, 1, 3)); pos = np.clip(p + rng.normal(size=(n, 3, 3)) * 10 ** rng.uniform(-1.7, -0.5), 1.0, 4.0)
    nrm = rng.normal(size=(n, 3, 3)); nrm[..., 2] -= 2.0
    mats = [dict(ka=(1, 1, 1), kd=(0.8, 0.9, 1.0), ks=(0.5, 0.5, 0.5), ns=40.0, kr=0.5, tex=0, bump=-1)]
    return dict(pos=pos, uv=rng.random((n, 3, 3)), nrm=nrm, mat=np.zeros(n, np.uint32), materials=mats, textures=[checker((230, 200, 170), (60, 90, 160))], root=ROOT_BOX)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(30))
def test_random_small_scenes_match_the_oracle_frame(rrt, ob, seed):
    """Case 8."""
    A = _random_scene(seed)
    osc = oracle_for(ob, A, LIGHTS, CAMERA)
    ch = chains_of(osc.octree())
    n_rec = len(with_record(ch))
    if len(A["pos"]) >= 8:
        assert any(p == 0 and len(nodes) >= 2 for p, nodes, _, _ in ch), f"seed {seed}: no chain of two or more nodes below the root: {ch}"
    ref = osc.render(320, 240, n_threads=N_THREADS)[0]
    worst = 0
    for label, rt in _raytracers(rrt, A):
        assert rt.chain_info["n_chains"] == n_rec, (seed, label, rt.chain_info, n_rec)
        worst = max(worst, int(assert_frame_close(rt.render(320, 240), ref, f"seed {seed} ({len(A['pos'])} triangles), {label}", COLOUR_TOL).max()))
    print(f"\n[chain shortcut] seed {seed}: {len(A['pos'])} triangles, {len(ch)} chains, {n_rec} with a record, max channel diff {worst}")


@pytest.mark.gpu
def test_teapot_chains_records_and_frame(rrt, ob, teapot, teapot_oracle):
    """Case 9."""
    ch = chains_of(teapot_oracle.octree())
    below_root = [c for c in ch if c[0] == 0]
    assert len(below_root) == 4 and sum(len(c[1]) for c in below_root) == 8, below_root                 # the four chains 5-11, 6-84, 7-57, 8-34 below the root
    assert [(c[1], c[2]) for c in below_root] == [([5, 11], 19), ([6, 84], 92), ([7, 57], 65), ([8, 34], 42)], below_root
    assert all(len(c[3]) == 2 for c in below_root)
    rec = with_record(ch)
    assert (len(ch), len(rec), sum(len(c[1]) for c in rec)) == (63, 24, 30), (len(ch), len(rec))
    lights = rrt.default_lights()
    gpu = rrt.RayTracer(teapot, lights, box_filter="bundle"); host = rrt.RayTracer(teapot, lights, box_filter="bundle", host_setup=True)
    off = rrt.RayTracer(teapot, lights, box_filter="bundle", chain_shortcut=False)
    for rt in (gpu, host, off):
        assert rt.chain_info == {"n_chains": len(rec), "n_chain_nodes": sum(len(c[1]) for c in rec)}, rt.chain_info
    g, h = gpu.buffer("chains"), host.buffer("chains")
    assert g.shape == h.shape == (160 * len(rec),) and np.array_equal(g, h), "chain records of the GPU set-up and the host set-up differ"
    assert np.array_equal(gpu.buffer("child_boxes"), host.buffer("child_boxes"))
    ends = sorted(int(e) for e in g.view(np.uint32).reshape(-1, 40)[:, 6])
    assert ends == sorted(c[2] for c in rec), (ends, "end nodes of the records")
    a, b = gpu.render(1920, 1080), off.render(1920, 1080)
    assert np.array_equal(a, b), f"{(a != b).sum()} pixels of the 1080p frame differ with the shortcut"
    assert np.array_equal(a, host.render(1920, 1080))
