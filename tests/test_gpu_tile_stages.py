"""The deferred stages over a device-resident tile list on the GPU (include/rrt.h: rrt_render_visibility_tile_list_device, rrt_render_surface_tile_list_device,
rrt_shade_surface_tile_list_device, rrt_ambient_surface_tile_list_device).

The statement under test: inside the tiles a list names, every requested output holds what the region call of the same name writes for the whole frame
(region=None), bit for bit, in every traversal variant; outside them, and behind the planes' ends, nothing is written; shading and ambient occlusion need their
input planes in the listed tiles only.  Every output lives in a buffer prefilled with 0xA5 bytes in front of a guard tail (tile_stage_checks.GuardedPlane), the
inputs of shade and ambient hold 0xA5 bytes outside the listed tiles, and every comparison is bitwise.assert_same_bits.

The frame is 203 x 117 (390 tiles): partial tiles on the right and at the bottom, the untraced last column of an odd width, the untraced rows 0 and 1 of an odd
height.  9 x 9 is four tiles, all partial; 64 x 48 has whole tiles only.
"""
import numpy as np
import pytest

from ambient_checks import T8, T8_MAX_T
from bitwise import assert_same_bits
from gpu_checks import ALL_MODES
from region_render_checks import assert_frame_has_content, listed_pixels, tiles_of
from scenes import EYE3, H3, TARGET, W3, teapot_arrays  # noqa: F401  (fixture: teapot_arrays)
from shade_checks import soup_scene
from tile_stage_checks import (AMB_IN, DEAD, PLANES, SHADE_IN, T1, T32, TEN, VIS, as_signed, assert_listed_only, device_list, device_plane, guarded, inputs_for,
                               lists_of, tensors)

pytestmark = pytest.mark.gpu

SIZES = ((W3, H3), (9, 9), (64, 48))
STAGES = ("visibility", "surface", "shade", "ambient")
AMBIENT_TABLES = {1: T1, 32: T32}


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


class Reference:
    """A raytracer in one walk mode at EYE3 and, per frame size, what the region calls give for the whole frame: the ten planes (one surface call), the frame
    shaded from them with and without the mask, the ambient outputs per table.  Computed once, read-only."""

    def __init__(self, rrt, sd, mode, look=True):
        self.rt = rrt.RayTracer(sd, rrt.default_lights(), box_filter=mode)
        if look:
            self.rt.look_at(EYE3, TARGET)
        self.mode, self._sizes = mode, {}

    def at(self, w, h):
        if (w, h) not in self._sizes:
            rt = self.rt
            full = rt.surface(w, h, visibility=VIS)
            full["fb"] = rt.shade(w, h, full)
            full["fb without the mask"] = rt.shade(w, h, {n: a for n, a in full.items() if n != "lights"})
            for n, table in AMBIENT_TABLES.items():
                out = rt.ambient(w, h, full, table, T8_MAX_T)
                full[f"occluded {n}"], full[f"grey {n}"] = out["occluded"], out["grey"]
            for a in full.values():
                a.setflags(write=False)
            self._sizes[(w, h)] = full
        return self._sizes[(w, h)]


_references = {}


@pytest.fixture(scope="module")
def reference(rrt, teapot):
    def get(mode):
        if mode not in _references:
            _references[mode] = Reference(rrt, teapot, mode)
        return _references[mode]
    yield get
    _references.clear()


def run_stage(torch, rt, stage, full, w, h, tiles_t, listed, bound_t=None, stream=None, what=""):
    """Every variant of one stage over the list, each into fresh guarded planes: [(what, {plane: GuardedPlane}, {plane: the whole-frame reference})].  listed: the
    entries that count; the inputs of shade and ambient hold the kept planes in those tiles only."""
    out = []
    poison = lambda names: inputs_for(torch, names, full, w, h, listed)
    kw = dict(stream=stream, bound_t=bound_t)
    if stage == "visibility":
        g = guarded(torch, VIS, w, h)
        rt.visibility_tile_list_into(tensors(g), tiles_t, w, h, **kw)
        out.append((f"{what}: all six planes", g, full))
    elif stage == "surface":
        for names in (TEN, ("lights",)):
            g = guarded(torch, names, w, h)
            rt.surface_tile_list_into(tensors(g), tiles_t, w, h, **kw)
            out.append((f"{what}: planes {names}", g, full))
    elif stage == "shade":
        for names, key in ((SHADE_IN, "fb"), (SHADE_IN[:4], "fb without the mask")):
            g = guarded(torch, ("fb",), w, h)
            rt.shade_tile_list_into(g["fb"].t, poison(names), tiles_t, w, h, **kw)
            out.append((f"{what}: {key}", g, {"fb": full[key]}))
    else:
        for n, table in AMBIENT_TABLES.items():
            for names in (("occluded",), ("grey",), ("occluded", "grey")):
                g = guarded(torch, names, w, h)
                rt.ambient_tile_list_into(tensors(g), poison(AMB_IN), table, T8_MAX_T, tiles_t, w, h, **kw)
                out.append((f"{what}: n = {n}, outputs {names}", g, {"occluded": full[f"occluded {n}"], "grey": full[f"grey {n}"]}))
    return out


def assert_reference_has_content(full, w, h, what):
    """A comparison of misses with misses shows nothing: the frame holds shaded pixels, hits, lit and dark lights, open and occluded hemisphere rays."""
    if w * h < 64 * 48:
        return
    assert_frame_has_content(full["fb"], what)
    hit = full["hit"].astype(bool)
    assert hit.mean() > 0.2 and (~hit).any(), f"{what}: {hit.mean():.2f} of the sub-samples hit"
    assert len(np.unique(full["lights"][hit])) >= 2, f"{what}: every hit sees the same lights"
    assert len(np.unique(full["occluded 32"][hit])) >= 2, f"{what}: the hemisphere rays of every hit give the same mask"


# ------------------------------------------------------------------ 1: each stage against its region twin
@pytest.mark.parametrize("mode", ALL_MODES)
@pytest.mark.parametrize("stage", STAGES)
def test_a_stage_over_a_list_is_its_region_twin_in_the_listed_tiles(torch, reference, stage, mode):
    assert_the_lists_are_what_their_names_say()
    ref = reference(mode)
    for w, h in SIZES:
        full = ref.at(w, h)
        assert_reference_has_content(full, w, h, f"walk {mode}: teapot {w}x{h}")
        for name, tiles in lists_of(w, h).items():
            what = f"walk {mode}, {w}x{h}, {stage}, {name} ({len(tiles)} entries)"
            runs = run_stage(torch, ref.rt, stage, full, w, h, device_list(torch, tiles), tiles, what=what)
            torch.cuda.synchronize()
            for case, planes, want in runs:
                n_px = assert_listed_only(planes, want, w, h, tiles, case)
            assert (n_px == 0) == (len(tiles) == 0) and (n_px == w * h or not name.startswith("every tile")), f"{what}: {n_px} listed pixels"


def assert_the_lists_are_what_their_names_say():
    """(of the test's own lists, on the frame with 390 tiles)"""
    L = lists_of(W3, H3)
    tx, ty = tiles_of(W3, H3)
    n = tx * ty
    assert n == 390 and len(L) == 7
    assert (L["every tile, ascending"] == np.arange(n)).all() and (L["every tile, descending"] == np.arange(n)[::-1]).all()
    q = L["a seeded quarter"]
    assert len(q) == 97 == len(set(q.tolist())) and q.max() < n and (np.diff(q.astype(np.int64)) < 0).any()
    rim = L["the corners and the edges"]
    assert rim[:4].tolist() == [0, tx - 1, n - tx, n - 1] and len(rim) == len(set(rim.tolist())) == 2 * tx + 2 * ty - 4
    assert all(t % tx in (0, tx - 1) or t // tx in (0, ty - 1) for t in rim.tolist())
    d = L["duplicates"]
    assert len(d) == 2 * 48 + 1 and len(set(d.tolist())) == 48
    m = L["invalid entries interleaved"]
    assert (m[0::2] == q).all() and set(m[1::2].tolist()) == {DEAD, n, n + 1}
    assert len(L["the empty list"]) == 0
    assert len(lists_of(9, 9)["every tile, ascending"]) == 4


# ------------------------------------------------------------------ 2: the bound
@pytest.mark.parametrize("mode", ALL_MODES)
def test_the_bound_is_read_on_the_device_and_ends_the_list(torch, reference, mode):
    """Entries at and beyond m = min(n, *d_count) name valid tiles of their own, whose pixels stay 0xA5.  In the last case torch writes the count on the call's
    stream, which is not the default one, just before the call, with no synchronisation in between."""
    ref = reference(mode)
    w, h = W3, H3
    full = ref.at(w, h)
    n = 40
    tiles = np.random.default_rng(17).permutation(390)[:n].astype(np.uint32)
    tiles_t = device_list(torch, tiles)
    for stage in STAGES:
        for count in (None, 0, 1, 23, n, n + 1, 0xFFFFFFFF):
            m = n if count is None else min(n, count)
            bound_t = None if count is None else torch.from_numpy(np.array([count], np.uint32).view(np.int32)).cuda()
            what = f"walk {mode}, {stage}, n = {n}, count {count}"
            runs = run_stage(torch, ref.rt, stage, full, w, h, tiles_t, tiles[:m], bound_t, what=what)
            torch.cuda.synchronize()
            for case, planes, want in runs:
                assert assert_listed_only(planes, want, w, h, tiles[:m], case) == int(listed_pixels(w, h, tiles[:m]).sum())
        # the count written by torch on the same non-default stream
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            bound_t = torch.full((1,), n, dtype=torch.int32, device="cuda")
            seven = torch.full((1,), 7, dtype=torch.int32, device="cuda")
            for _ in range(8):                               # (work in front of the write, so that a kernel that did not wait would run first)
                bound_t.add_(seven).sub_(seven)
            bound_t.sub_(n - 7)
            runs = run_stage(torch, ref.rt, stage, full, w, h, tiles_t, tiles[:7], bound_t, stream=stream.cuda_stream, what=f"walk {mode}, {stage}, count written on the stream")
        torch.cuda.synchronize()
        for case, planes, want in runs:
            assert_listed_only(planes, want, w, h, tiles[:7], case)


# ------------------------------------------------------------------ 3: a tex / bump edit, repaired twice on one stream
def select(rrt, torch, rt, test, w, h):
    """(list, count) tensors of one select call on the current stream"""
    tx, ty = tiles_of(w, h)
    n = tx * ty
    lst, cnt = torch.full((n,), 0x25, dtype=torch.int32, device="cuda"), torch.full((1,), 0x25, dtype=torch.int32, device="cuda")
    marks = torch.zeros(n, dtype=torch.uint8, device="cuda")
    scratch = torch.empty(rrt.compact_scratch_bytes(n), dtype=torch.uint8, device="cuda")
    rt.select_tiles_into(lst, cnt, marks, scratch, [test], w, h)
    return lst, cnt


@pytest.mark.parametrize("mode", ALL_MODES)
def test_a_texture_edit_repaired_through_tile_lists_round_after_round(rrt, torch, teapot, mode):
    """Frame and ten planes kept on the device.  Round 1: material 0 (the teapot) gets the tex and bump of material 1; A = SET{0} over the kept material plane,
    B = SET{0, 3} (3 is the only mirror); the surface stage over A into all ten planes, the shade stage over B with the mask into the old frame, nothing read
    back in between: the frame is a fresh render and the planes are a fresh surface launch.  Round 2, from the repaired planes: material 1 gets the tex and bump
    of material 2 in the same way.  No triangle of the teapot scene has material 1, so A is empty there and B is the mirror's tiles: the round shows that the
    repaired planes serve a second selection and a second shading.  Round 3 edits material 2, which is in view, in the same way again."""
    rt = rrt.RayTracer(teapot, rrt.default_lights(), box_filter=mode)
    rt.look_at(EYE3, TARGET)
    w, h = W3, H3
    fb = torch.zeros(w * h, dtype=torch.int32, device="cuda")
    kept = {n: device_plane(torch, n, w, h) for n in TEN}
    rt.render_into(fb, w, h)
    rt.surface_into(kept, w, h)
    torch.cuda.synchronize()
    old = fb.cpu().numpy().view(np.uint32).reshape(h, w).copy()
    assert_frame_has_content(old, f"walk {mode}: teapot {w}x{h} at {EYE3}")
    mats = rt.materials()
    assert [k for k, m in enumerate(mats) if m["kr"] > 0] == [3], "material 3 is the scene's only mirror"
    for rnd, (edited, donor) in enumerate(((0, 1), (1, 2), (2, 0)), 1):
        what = f"walk {mode}, round {rnd} (material {edited} takes tex and bump of {donor})"
        assert (mats[edited]["tex"], mats[edited]["bump"]) != (mats[donor]["tex"], mats[donor]["bump"]), what
        mats[edited] = dict(mats[edited], tex=mats[donor]["tex"], bump=mats[donor]["bump"])
        rt.set_materials(mats)
        list_a, count_a = select(rrt, torch, rt, rrt.tile_test("set", kept["material"], values=(edited,)), w, h)
        list_b, count_b = select(rrt, torch, rt, rrt.tile_test("set", kept["material"], values=(edited, 3)), w, h)
        rt.surface_tile_list_into(kept, list_a, w, h, bound_t=count_a)
        rt.shade_tile_list_into(fb, kept, list_b, w, h, bound_t=count_b)
        torch.cuda.synchronize()
        a, b = int(count_a.cpu().numpy().view(np.uint32)[0]), int(count_b.cpu().numpy().view(np.uint32)[0])
        fresh, planes = rt.render(w, h), rt.surface(w, h, visibility=VIS)
        changed = int((fresh != old).sum())
        print(f"{what}: |A| = {a}, |B| = {b} of 390 tiles; the edit changes {changed} pixels")
        if rnd == 1:
            assert 0 < a <= b < 390, f"{what}: |A| = {a}, |B| = {b}"
            assert changed >= 64, f"{what}: the edit changes {changed} pixels"
        if rnd == 3:
            assert 0 < a <= b < 390 and changed >= 1, f"{what}: |A| = {a}, |B| = {b}, {changed} pixels changed"
        assert_same_bits(fb.cpu().numpy().view(np.uint32).reshape(h, w), fresh, f"{what}: the repaired frame vs a fresh render", np.uint32)
        for n in TEN:
            assert_same_bits(kept[n].cpu().numpy().view(PLANES[n][0]), planes[n], f"{what}: the repaired plane {n} vs a fresh surface launch", PLANES[n][0])
        old = fresh


# ------------------------------------------------------------------ 4: adaptive ambient occlusion
@pytest.mark.parametrize("mode", ALL_MODES)
def test_more_ambient_samples_where_the_first_eight_disagree(rrt, torch, reference, mode):
    """8 directions everywhere (ambient_checks.T8, max_t = T8_MAX_T = 2.0) -> RANGE 1 <= occluded < 255 selects the tiles in which some hit's eight rays are
    neither all open nor all blocked -> tile_stage_checks.T32, whose first eight directions are T8, on those tiles only, into a second `occluded` plane and a grey
    plane: the whole-frame n = 32 call in the listed tiles, 0xA5 elsewhere.
    Checked on the CPU before these values were fixed, with the oracle's intersector alone (surface_checks.expected_planes and ambient_checks.by_oracle at
    203 x 117 from EYE3): T8 with max_t = 2.0 selects 269 of the 390 tiles (51 581 elements in [1, 255), 12 800 equal to 255, 1 833 hits with 0)."""
    ref = reference(mode)
    rt, w, h = ref.rt, W3, H3
    full = ref.at(w, h)
    assert (T32[:8] == T8).all() and len(T32) == 32
    kept = {n: torch.from_numpy(as_signed(full[n])).cuda() for n in AMB_IN}
    first = guarded(torch, ("occluded",), w, h)
    rt.ambient_into({"occluded": first["occluded"].t}, kept, T8, T8_MAX_T, w, h)
    lst, cnt = select(rrt, torch, rt, rrt.tile_test("range", first["occluded"].t, lo=1, hi=255), w, h)
    second = guarded(torch, ("occluded", "grey"), w, h)
    rt.ambient_tile_list_into(tensors(second), kept, T32, T8_MAX_T, lst, w, h, bound_t=cnt)
    torch.cuda.synchronize()
    want8 = rt.ambient(w, h, full, T8, T8_MAX_T, outputs=("occluded",))["occluded"]
    assert_same_bits(first["occluded"].host("n = 8"), want8, f"walk {mode}: the whole-frame n = 8 launch", np.uint32)
    passing = ((want8 >= 1) & (want8 < 255)).any(-1)
    tx, ty = tiles_of(w, h)
    marks = np.zeros((ty, tx), bool)
    ys, xs = np.nonzero(passing)
    marks[ys // 8, xs // 8] = True
    count = int(cnt.cpu().numpy().view(np.uint32)[0])
    print(f"walk {mode}: {count} of 390 tiles hold a hit whose eight rays disagree")
    assert 0 < int(marks.sum()) < 390, f"{int(marks.sum())} of 390 tiles selected by the reference planes"
    tiles = lst.cpu().numpy().view(np.uint32)
    assert_same_bits(tiles[:count], np.flatnonzero(marks.reshape(-1)).astype(np.uint32), f"walk {mode}: the selected tiles", np.uint32)
    assert_listed_only(second, {"occluded": full["occluded 32"], "grey": full["grey 32"]}, w, h, tiles[:count], f"walk {mode}: n = 32 on the selected tiles")
    mask = listed_pixels(w, h, tiles[:count])
    assert_same_bits(second["occluded"].host("n = 32")[mask] & np.uint32(0xFF), want8[mask], f"walk {mode}: the low eight bits of n = 32 are n = 8", np.uint32)


# ------------------------------------------------------------------ 5: after set_camera and after set_triangles
@pytest.mark.parametrize("mode", ALL_MODES)
def test_visibility_of_the_tiles_that_differ_after_a_move(rrt, torch, teapot, mode):
    """Old planes kept; the camera moves (then the triangles do); the fresh `t` plane is taken; DIFFERS over old and new `t` selects; the visibility stage over
    that list gives the fresh planes in those tiles -- and laid over the old `t` plane, the fresh `t` plane everywhere."""
    rt = rrt.RayTracer(teapot, rrt.default_lights(), box_filter=mode)
    rt.look_at(EYE3, TARGET)
    w, h = W3, H3
    old = rt.visibility(w, h)
    pos, uv, nrm, mat = teapot.triangles()

    def move_camera():
        rt.look_at((-6.5, 4.0, -6.5), TARGET)

    def move_triangles():
        rt.set_triangles(pos + np.array([0.25, 0.0, 0.125]), uv, nrm, mat)

    for name, move in (("set_camera", move_camera), ("set_triangles", move_triangles)):
        what = f"walk {mode}, after {name}"
        move()
        fresh = rt.visibility(w, h)
        old_t, new_t = torch.from_numpy(old["t"].copy()).cuda(), torch.from_numpy(fresh["t"].copy()).cuda()
        lst, cnt = select(rrt, torch, rt, rrt.tile_test("differs", old_t, new_t), w, h)
        g = guarded(torch, VIS, w, h)
        rt.visibility_tile_list_into(tensors(g), lst, w, h, bound_t=cnt)
        rt.visibility_tile_list_into({"t": old_t}, lst, w, h, bound_t=cnt)
        torch.cuda.synchronize()
        count = int(cnt.cpu().numpy().view(np.uint32)[0])
        tiles = lst.cpu().numpy().view(np.uint32)[:count]
        differs = (old["t"].view(np.uint64) != fresh["t"].view(np.uint64)).any(-1)
        print(f"{what}: {count} of 390 tiles differ in t, {int(differs.sum())} pixels")
        assert 0 < count and int(differs.sum()) >= 64, f"{what}: {count} tiles, {int(differs.sum())} pixels differ"
        assert not (differs & ~listed_pixels(w, h, tiles)).any(), f"{what}: a pixel that differs lies outside the selected tiles"
        assert_listed_only(g, fresh, w, h, tiles, what)
        assert_same_bits(old_t.cpu().numpy(), fresh["t"], f"{what}: the old t plane with the listed tiles laid over it", np.float64)
        old = fresh


# ------------------------------------------------------------------ 6: a scene with group records
@pytest.mark.parametrize("mode", ALL_MODES)
def test_the_four_stages_on_a_soup_with_group_records(rrt, torch, teapot_arrays, mode):  # noqa: F811
    """The 4 000-triangle soup of tests/test_gpu_surface.py, whose long own lists carry group records: the kernels' group instantiations."""
    A = soup_scene(teapot_arrays)
    sd = rrt.SceneData.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], A["materials"], A["textures"])
    ref = Reference(rrt, sd, mode, look=False)
    supers = ref.rt.buffer("supers").view(np.uint32).reshape(-1, 8)
    assert len(supers) > 0 and (supers[:, 7] == 0).any(), "no own list of this soup is long enough for group records: the kernels' group instantiation did not run"
    w, h = 64, 48
    full = ref.at(w, h)
    assert_reference_has_content(full, w, h, f"walk {mode}: soup {w}x{h}")
    tiles = lists_of(w, h)["a seeded quarter"]
    for stage in STAGES:
        what = f"walk {mode}, soup {w}x{h}, {stage}, a seeded quarter ({len(tiles)} entries)"
        runs = run_stage(torch, ref.rt, stage, full, w, h, device_list(torch, tiles), tiles, what=what)
        torch.cuda.synchronize()
        for case, planes, want in runs:
            assert assert_listed_only(planes, want, w, h, tiles, case) == 64 * len(tiles)
