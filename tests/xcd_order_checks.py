"""Helpers of the tests of the XCD-aware block order (csrc/render.hip: render_kernel and stage_lane(const Region&); csrc/frames.cpp: frame_params): the
re-labelling restated, the grid of every kind of launch that takes it, the case table that parent and child share, and `collect`, which runs every case in the
current process and returns every output under a stable name.

A wrong re-labelling computes nothing wrong: it runs some blocks twice and others never, or reads the coverage bit of another wave.  So every output of
`collect` goes into device memory whose every byte is 0xA5 before the call, in front of a guard tail that is checked after it (tile_stage_checks.GuardedPlane; a
frame or a rank's tiles are a plane "fb" of the right shape).  A block that never ran leaves 0xA5 behind.  Every call is a device (`*_into`) form, with two
exceptions the library has no device form of: render_progressive, whose bands are the fourth kind of launch -- it clears its device frame to 0 on every call, and
0 is no pixel of a traced hit or of the background -- and pick, a one-tile region launch of four blocks, which no chunk re-labels (full == 0).

The order in force is the process's: RRT_XCD_CHUNK is read once, by the first frame_params.  Nothing here sets or reads it.

Plain module, not a test module: pytest does not rewrite its asserts, so every assert here states both values in its message.  It holds no fixtures.
"""
import importlib
import os

import numpy as np

from ambient_checks import T8, T8_MAX_T, traced_mask
from conftest import ASSETS
from gpu_checks import ALL_MODES, FORCED_MODES
from region_render_checks import tiles_of
from scenes import EYE3, H3, TARGET, W3, arrays_of
from shade_checks import soup_scene
from tile_stage_checks import FILL, TEN, VIS, GuardedPlane, guarded, tensors

ENV = "RRT_XCD_CHUNK"                                      # csrc/frames.cpp: frame_params
FORCED_CHUNKS = (2, 5, 7)                                  # (1 is the identity: relabel(b, g, 1) == b)
DEFAULT_CHUNK, DEFAULT_FROM = 256, 50000                   # frame_params: chunk 256 for scenes of 50 000 triangles in the tree and more


# ------------------------------------------------------------------ the formula (render.hip, the same four lines in render_kernel and stage_lane(const Region&))
def full_blocks(grid, chunk):
    """full = (gridDim.x / (8 C)) * (8 C): the blocks that are permuted; 0 with C = 0, the plain order."""
    return (grid // (8 * chunk)) * (8 * chunk) if chunk else 0


def relabel(blk, grid, chunk):
    """The label a block takes: below `full`, xcd = blk & 7, i = blk >> 3, blk = ((i / C) * 8 + xcd) * C + (i % C); in the tail, its own index."""
    blk = np.asarray(blk, np.int64)
    if not chunk:
        return blk.copy()
    xcd, i = blk & 7, blk >> 3
    return np.where(blk < full_blocks(grid, chunk), ((i // chunk) * 8 + xcd) * chunk + (i % chunk), blk)


# ------------------------------------------------------------------ the grid of each kind of launch: one block per quadrant of a tile
def frame_grid(w, h):
    """A whole frame (render.hip: launch_render, world 1): 4 * tiles."""
    tx, ty = tiles_of(w, h)
    return 4 * tx * ty


def share_grid(w, h, world):
    """A rank's share (launch_render: local_tiles = ceil(tiles / world)), the same for every rank: the last blocks of some ranks name no tile."""
    tx, ty = tiles_of(w, h)
    return 4 * ((tx * ty + world - 1) // world)


def region_grid(w, h, region):
    """A region (regions.cpp: in_region): four times the tile rectangle from tile (x0 / 8, y0 / 8) to the tiles that hold the region's last column and row."""
    x0, y0, rw, rh = (0, 0, w, h) if region is None else region
    return 4 * ((x0 + rw + 7) // 8 - x0 // 8) * ((y0 + rh + 7) // 8 - y0 // 8)


def band_grids(w, h, chunk_rows):
    """The launches of render_progressive, first to last (frames.cpp: rrt_render_progressive, the loop `for (int64_t cs = -half; cs < half; cs += chunk_rows)` and
    the five lines under it): scene rows [cs, ce) are canvas rows r_lo .. r_hi, the launch takes the whole tile rows that hold them, tile_begin = (row_begin / 8)
    * tiles_x to tile_end = ((row_end + 7) / 8) * tiles_x, and launch_render gives it 4 * (tile_end - tile_begin) blocks."""
    tx, _ = tiles_of(w, h)
    half, grids = h // 2, []
    for cs in range(-half, half, chunk_rows):
        ce = min(cs + chunk_rows, half)
        r_lo, r_hi = h - (ce - 1 + half), min(h - (cs + half), h - 1)
        if r_lo <= r_hi:
            row_begin, row_end = r_lo, r_hi + 1
            grids.append(4 * (((row_end + 7) // 8) * tx - (row_begin // 8) * tx))
    return grids


# ------------------------------------------------------------------ the case table, shared by parent and child
POSES = ("creation pose", f"eye {EYE3}")
SIZES = ((64, 48), (W3, H3), (9, 9))                       # whole tiles only; partial tiles right and bottom, odd width and height; four partial tiles
WORLD = 3
BAND_ROWS = {(W3, H3): (16, 50), (9, 9): (16,)}            # chunk_rows of render_progressive per size (9 x 9: one band of 16 blocks, the only band with full == 0)
ONE_TILE_REGIONS = ((200, 0, 3, 2), (8, 8, 8, 8))          # 4 blocks: full == 0 for every chunk
REGIONS = {(W3, H3): (None, (13, 50, 77, 31)) + ONE_TILE_REGIONS, (64, 48): (None,), (9, 9): (None,)}
SOUP_SIZE, SOUP_REGIONS = (64, 48), (None, (8, 8, 40, 24))
SOUP_MODES = ALL_MODES
LARGE_TRIS, LARGE_SEED = 60000, 0x5EED0003
LARGE_SIZE = (264, 136)                                    # 33 x 17 = 561 tiles, 2244 blocks: full = 2048 with chunk 256, a tail of 196
LARGE_REGIONS = (None, (8, 0, 256, 136))                   # 32 x 17 = 544 tiles, 2176 blocks: full = 2048, a tail of 128
LARGE_MODES = FORCED_MODES


def small_grids():
    """[(kind, what, grid)] of every launch of `collect` that takes the order, by the four kinds: frame, share, band, region."""
    out = []
    for w, h in SIZES:
        out.append(("frame", f"{w}x{h}", frame_grid(w, h)))
        out.append(("share", f"world {WORLD} of {w}x{h}", share_grid(w, h, WORLD)))
        for rows in BAND_ROWS.get((w, h), ()):
            out += [("band", f"band {k} of {w}x{h} in chunks of {rows} rows", g) for k, g in enumerate(band_grids(w, h, rows))]
        out += [("region", f"region {r} of {w}x{h}", region_grid(w, h, r)) for r in REGIONS[(w, h)]]
    out.append(("frame", "soup {}x{}".format(*SOUP_SIZE), frame_grid(*SOUP_SIZE)))
    out += [("region", "soup region {} of {}x{}".format(r, *SOUP_SIZE), region_grid(*SOUP_SIZE, r)) for r in SOUP_REGIONS]
    return out


def large_grids():
    return [("frame", "large soup {}x{}".format(*LARGE_SIZE), frame_grid(*LARGE_SIZE))] + \
           [("region", "large soup region {} of {}x{}".format(r, *LARGE_SIZE), region_grid(*LARGE_SIZE, r)) for r in LARGE_REGIONS]


# ------------------------------------------------------------------ running the cases
def package():
    return importlib.import_module("rust-ray-tracer_amd")


def u32(*values):
    return np.array(values, np.uint32)


def frame_into(torch, w, h):
    """A guarded [h][w] buffer of four-byte pixels, every byte 0xA5."""
    return GuardedPlane(torch, "fb", w, h)


def pose(rt, k):
    if k == 0:
        rt.reset_camera()
    else:
        rt.look_at(EYE3, TARGET)


def frames(rrt, torch, out, key, rt_off, rt_always, w, h):
    """render_into without the coverage pass and with it; with it, also the mask the frame ran with and the state of the pass."""
    fb = frame_into(torch, w, h)
    rt_off.render_into(fb.t, w, h)
    out[f"{key}, render_into coverage=False"] = fb.host(key)
    fb = frame_into(torch, w, h)
    rt_always.render_into(fb.t, w, h)
    out[f"{key}, render_into coverage=always"] = fb.host(key)
    state = rt_always.coverage_info()["state"]
    out[f"{key}, coverage state"] = u32(rrt.COVERAGE_STATES.index(state))
    mask = rt_always.coverage_mask()
    if mask is not None:
        out[f"{key}, coverage mask"] = mask


def shares(torch, out, key, rt, w, h):
    """Every rank's tiles of a world of WORLD, padding included, each into a buffer of its own; the gathered buffer de-tiled."""
    tx, ty = tiles_of(w, h)
    per_rank = (tx * ty + WORLD - 1) // WORLD
    ranks = []
    for rank in range(WORLD):
        g = GuardedPlane(torch, "fb", 64, per_rank)       # [tiles of the rank][64 pixels]
        rt.render_tiles_into(g.t.view(-1), w, h, rank, WORLD)
        out[f"{key}, tiles of rank {rank} of {WORLD}"] = g.host(f"{key}, rank {rank}")
        ranks.append(g.t.view(-1))
    fb = frame_into(torch, w, h)
    rt.detile_into(torch.cat(ranks).contiguous(), fb.t.view(-1), w, h, WORLD)
    out[f"{key}, de-tiled frame of {WORLD} ranks"] = fb.host(f"{key}, detile")


def region_calls(torch, out, key, rt, w, h, region):
    """The five region calls of one region: visibility (six planes), surface (ten planes), shade from those ten with the mask, ambient from them (both outputs)
    and the fused frame of the region.  Returns the surface call's planes in host memory."""
    rw, rh = (w, h) if region is None else region[2:]
    key = f"{key}, region {region}"
    vis = guarded(torch, VIS, rw, rh)
    rt.visibility_into(tensors(vis), w, h, region)
    for n, p in vis.items():
        out[f"{key}, visibility_into {n}"] = p.host(key)
    ten = guarded(torch, TEN, rw, rh)
    rt.surface_into(tensors(ten), w, h, region)
    host = {n: p.host(key) for n, p in ten.items()}
    for n, a in host.items():
        out[f"{key}, surface_into {n}"] = a
    fb = frame_into(torch, rw, rh)
    rt.shade_into(fb.t, tensors(ten), w, h, region)
    out[f"{key}, shade_into with the mask"] = fb.host(key)
    amb = guarded(torch, ("occluded", "grey"), rw, rh)
    rt.ambient_into(tensors(amb), tensors(ten), T8, T8_MAX_T, w, h, region)
    for n, p in amb.items():
        out[f"{key}, ambient_into {n}"] = p.host(key)
    fb = frame_into(torch, rw, rh)
    rt.render_region_into(fb.t, w, h, region)
    out[f"{key}, render_region_into"] = fb.host(key)
    return host


def picks(out, key, rt, w, h, hit):
    """pick at the first traced pixel whose sub-sample 0 hits and at the first whose sub-sample 0 misses, by the surface call's `hit` plane of the whole frame
    (where the frame has such a pixel); the pixel is part of the output."""
    traced = traced_mask(w, h)
    for name, which in (("hit", traced & (hit[..., 0] != 0)), ("miss", traced & (hit[..., 0] == 0))):
        at = np.argwhere(which)
        if len(at):
            py, px = (int(v) for v in at[0])
            r = rt.pick(w, h, px, py)
            out[f"{key}, pick of a {name}, pixel hit tri albedo"] = u32(px, py, int(r["hit"]), r["tri"], r["albedo"])
            out[f"{key}, pick of a {name}, t u v"] = np.array([r["t"], r["u"], r["v"]], np.float64)


def root_count(rt):
    """The root's triangle_count (octree.rs:75): the triangles in the tree, what frame_params compares with 50 000."""
    return int(rt.octree()["tri_count"][0])


def collect_teapot(rrt, torch, out):
    sd = rrt.parse_obj_file(os.path.join(ASSETS, "model2.obj"))
    for mode in ALL_MODES:
        rt_off = rrt.RayTracer(sd, rrt.default_lights(), box_filter=mode, coverage=False)
        rt_always = rrt.RayTracer(sd, rrt.default_lights(), box_filter=mode, coverage="always")
        out["teapot, root triangle_count"] = u32(root_count(rt_off))
        for k, pose_name in enumerate(POSES):
            pose(rt_off, k)
            pose(rt_always, k)
            for w, h in SIZES:
                key = f"teapot, walk {mode}, {pose_name}, {w}x{h}"
                frames(rrt, torch, out, key, rt_off, rt_always, w, h)
                for rows in BAND_ROWS.get((w, h), ()):
                    out[f"{key}, render_progressive in chunks of {rows} rows"] = rt_off.render_progressive(w, h, chunk_rows=rows)
                shares(torch, out, key, rt_off, w, h)
                for region in REGIONS[(w, h)]:
                    host = region_calls(torch, out, key, rt_off, w, h, region)
                    if region is None:
                        picks(out, key, rt_off, w, h, host["hit"])
    return sd


def collect_soup(rrt, torch, out, teapot_sd):
    A = soup_scene(arrays_of(teapot_sd))
    sd = rrt.SceneData.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], A["materials"], A["textures"])
    w, h = SOUP_SIZE
    for mode in SOUP_MODES:
        rt = rrt.RayTracer(sd, rrt.default_lights(), box_filter=mode, coverage=False)
        supers = rt.buffer("supers").view(np.uint32).reshape(-1, 8)
        assert len(supers) > 0 and (supers[:, 7] == 0).any(), "no own list of this soup is long enough for group records: the kernels' group instantiation did not run"
        out["soup, root triangle_count"] = u32(root_count(rt))
        key = f"soup, walk {mode}, {w}x{h}"
        fb = frame_into(torch, w, h)
        rt.render_into(fb.t, w, h)
        out[f"{key}, render_into"] = fb.host(key)
        for region in SOUP_REGIONS:
            region_calls(torch, out, key, rt, w, h, region)


def collect(rrt, torch):
    """{name: array} of every small case, in the order in force in this process."""
    out = {}
    collect_soup(rrt, torch, out, collect_teapot(rrt, torch, out))
    torch.cuda.synchronize()
    return out


def large_scene(rrt):
    """The arrays of the 60 000-triangle soup: synthetic.soup_arrays, all of it inside the root box, the teapot's materials in turn and its textures."""
    syn = importlib.import_module("rust-ray-tracer_amd.synthetic")
    teapot = rrt.parse_obj_file(os.path.join(ASSETS, "model2.obj"))
    verts, vt, nrm = syn.soup_arrays(LARGE_TRIS, LARGE_SEED)
    assert np.abs(verts).max() < 20.0, f"a vertex of the soup lies outside the root box: {np.abs(verts).max()}"
    mats = teapot.materials()
    return dict(pos=verts, uv=np.concatenate([vt, np.zeros((LARGE_TRIS, 3, 1))], -1), nrm=np.repeat(nrm[:, None], 3, 1),
                mat=(np.arange(LARGE_TRIS) % len(mats)).astype(np.uint32), materials=mats, textures=teapot.textures())


def collect_large(rrt, torch):
    """{name: array} of the cases on the 60 000-triangle soup, in the order in force in this process."""
    out = {}
    A = large_scene(rrt)
    w, h = LARGE_SIZE
    for mode in LARGE_MODES:
        make = lambda coverage: rrt.RayTracer.from_arrays(A["pos"], A["uv"], A["nrm"], A["mat"], A["materials"], A["textures"], rrt.default_lights(),
                                                          box_filter=mode, coverage=coverage)
        rt_off, rt_always = make(False), make("always")
        out["large soup, root triangle_count"] = u32(root_count(rt_off))
        key = f"large soup, walk {mode}, {w}x{h}"
        frames(rrt, torch, out, key, rt_off, rt_always, w, h)
        for region in LARGE_REGIONS:
            region_calls(torch, out, key, rt_off, w, h, region)
    torch.cuda.synchronize()
    return out


COLLECTORS = {"small": collect, "large": collect_large}


# ------------------------------------------------------------------ what the plain-order outputs must hold for a comparison with them to show anything
def assert_outputs_have_content(out, rrt):
    """Of the outputs of `collect` or `collect_large`: no array still holds 0xA5 in every byte; the coverage pass was on at the two larger teapot sizes, and every
    mask there has proved-empty and walked waves; every pick of a hit is a hit and every pick of a miss a miss."""
    on = rrt.COVERAGE_STATES.index("on")
    n_masks = 0
    for name, a in out.items():
        if a.size > 4 and "pick" not in name and "triangle_count" not in name:
            assert not (np.ascontiguousarray(a).view(np.uint8) == FILL).all(), f"{name}: every byte is still {FILL:#x}"
        if name.startswith("teapot") and name.endswith("coverage state") and ", 9x9," not in name:
            assert int(a[0]) == on, f"{name}: {rrt.COVERAGE_STATES[int(a[0])]}, not on"
            mask = out[name[:-len("state")] + "mask"]
            n_masks += 1
            assert mask.any() and not mask.all(), f"{name}: {int(mask.sum())} of {mask.size} waves walked: a bit read for the wrong wave has nothing to change"
        if "pick of a" in name and name.endswith("albedo"):
            assert int(a[2]) == (1 if "pick of a hit" in name else 0), f"{name}: hit = {int(a[2])}"
    return n_masks
