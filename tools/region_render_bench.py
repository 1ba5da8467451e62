"""Developer tool: what the fused frame of a region (rrt_render_region_device) and of a device-resident tile list (rrt_render_tile_list_device) cost beside the
frame kernel they share a body with.  Per scene and per forced walk variant, HIP-event kernel_ms as the median of --launches launches after warm-up, with the
spread (min, max).  The launches of one group are taken in rotation -- a, b, c, a, b, c, ... -- so that what else runs on the machine meets all of them alike.
  (a) the whole frame: rrt_render_device of a raytracer with RRT_FLAG_NO_COVERAGE (the same walk over the same waves: the yardstick), rrt_render_region_device
      with the region = the whole frame, rrt_render_device with the coverage pass (the default), and rrt_render_tile_list_device of all tiles in order;
  (b) teapot only: the centre quarter and a 64 x 64 rectangle by rrt_render_region_device, beside rrt_render_surface_device (four surface planes and the albedo) +
      rrt_shade_surface_device (with the mask) of the same region;
  (c) the tile list: a seeded quarter of the tiles in ascending order, and 2 040 entries (8 160 blocks) that all leave at a bound of 0.
Every timed output is compared bit for bit with rrt_render_device's frame; a difference fails the run.
Scenes: the teapot and the 100 k-triangle soup, both at 1920 x 1080 in the creation pose.  One JSON: profiles/region_render.json.
   python tools/region_render_bench.py [--launches 20] [--scenes teapot,soup100k] [--out profiles/region_render.json]
Every scene is measured in a child process of its own under a time limit; the first failure stops the run."""
import argparse, importlib, json, os, statistics, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 1920, 1080
SCENES = {"teapot": 300, "soup100k": 420}       # time limit of the child, seconds
WARMUP = 3
QUARTER, SMALL = (480, 270, 960, 540), (928, 508, 64, 64)
EMPTY_ENTRIES = 2040                            # 8 160 blocks


def measure(scene, launches):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    rrt = importlib.import_module("rust-ray-tracer_amd"); syn = importlib.import_module("rust-ray-tracer_amd.synthetic")
    A = os.path.join(ROOT, "assets")
    sd = rrt.parse_obj_file(os.path.join(A, "model2.obj") if scene == "teapot" else syn.ensure_soup(A, 100000, syn.SEED_100K))
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device="cuda")
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device="cuda")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).cuda()
    tiles_x, tiles_y = (W + 7) // 8, (H + 7) // 8
    n_tiles = tiles_x * tiles_y
    every = dev(np.arange(n_tiles))
    some_ids = np.sort(np.random.default_rng(25).choice(n_tiles, n_tiles // 4, replace=False))
    some = dev(some_ids)
    listed = torch.zeros((tiles_y * 8, tiles_x * 8), dtype=torch.bool)
    for t in some_ids:
        listed[(t // tiles_x) * 8:(t // tiles_x) * 8 + 8, (t % tiles_x) * 8:(t % tiles_x) * 8 + 8] = True
    listed = listed[:H, :W].cuda()
    empty, zero = dev(np.arange(EMPTY_ENTRIES)), dev([0])

    def rotation(group):
        """{name: (raytracer, launch)} -> {name: median / min / max of kernel_ms}, the launches taken in rotation"""
        ms = {k: [] for k in group}
        for i in range(WARMUP + launches):
            for k, (rt, launch) in group.items():
                launch(); torch.cuda.synchronize()
                if i >= WARMUP: ms[k].append(rt.last_stats()["kernel_ms"])
        return {k: dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4)) for k, v in ms.items()}

    def same(got, want, what):
        if not torch.equal(got, want):
            raise SystemExit(f"{scene}: {what} differs from the frame of rrt_render_device on {int((got != want).sum())} pixels")

    m = lambda row, k: row[k]["median_ms"]
    out = dict(scene=scene, size=f"{W}x{H}", launches=launches, triangles=sd.info["n_tris"], tiles=n_tiles, walks={})
    for mode in ("lane", "bundle", "ray"):
        rt, bare = rrt.RayTracer(sd, rrt.default_lights(), box_filter=mode), rrt.RayTracer(sd, rrt.default_lights(), box_filter=mode, coverage=False)
        frame, covered, region, by_list = i32(H, W), i32(H, W), i32(H, W), i32(H, W)
        row = rotation({"frame_no_coverage": (bare, lambda: bare.render_into(frame, W, H)),
                        "region_whole_frame": (rt, lambda: rt.render_region_into(region, W, H)),
                        "frame_with_coverage_pass": (rt, lambda: rt.render_into(covered, W, H)),
                        "tile_list_all_in_order": (rt, lambda: rt.render_tile_list_into(by_list, every, W, H))})
        row["coverage_state_of_the_default_frame"] = rt.coverage_info()["state"]
        same(covered, frame, f"walk {mode}: the frame with the coverage pass"); same(region, frame, f"walk {mode}: the whole-frame region")
        same(by_list, frame, f"walk {mode}: the list of all tiles")
        f = row["frame_no_coverage"]
        row["region_over_frame_no_coverage"] = round(m(row, "region_whole_frame") / f["median_ms"], 3)
        row["region_within_the_frames_spread"] = bool(f["min_ms"] <= m(row, "region_whole_frame") <= f["max_ms"])
        row["region_over_frame_with_coverage_pass"] = round(m(row, "region_whole_frame") / m(row, "frame_with_coverage_pass"), 3)
        row["tile_list_over_region"] = round(m(row, "tile_list_all_in_order") / m(row, "region_whole_frame"), 3)
        # (c) a quarter of the tiles; blocks that all leave
        part, untouched = torch.full((H, W), -1, dtype=torch.int32, device="cuda"), torch.full((H, W), -1, dtype=torch.int32, device="cuda")
        row.update(rotation({"tile_list_quarter_of_the_tiles": (rt, lambda: rt.render_tile_list_into(part, some, W, H)),
                             "tile_list_8160_blocks_bound_0": (rt, lambda: rt.render_tile_list_into(untouched, empty, W, H, bound_t=zero))}))
        same(part, torch.where(listed, frame, torch.full_like(frame, -1)), f"walk {mode}: a quarter of the tiles")
        same(untouched, torch.full_like(frame, -1), f"walk {mode}: a list with a bound of 0")
        row["tile_list_quarter_over_all"] = round(m(row, "tile_list_quarter_of_the_tiles") / m(row, "tile_list_all_in_order"), 3)
        # (b) smaller regions beside the surface + shade pair
        if scene == "teapot":
            for name, (x0, y0, w, h) in (("centre_quarter", QUARTER), ("rect_64x64", SMALL)):
                planes = dict(point=f64(h, w, 4, 3), normal=f64(h, w, 4, 3), material=i32(h, w, 4), lights=i32(h, w, 4), albedo=i32(h, w, 4))
                fused, shaded = i32(h, w), i32(h, w)
                r = (x0, y0, w, h)
                sub = rotation({"region": (rt, lambda: rt.render_region_into(fused, W, H, region=r)),
                                "surface_all_planes_and_albedo": (rt, lambda: rt.surface_into(planes, W, H, region=r)),
                                "shade_with_mask": (rt, lambda: rt.shade_into(shaded, planes, W, H, region=r))})
                same(fused, frame[y0:y0 + h, x0:x0 + w], f"walk {mode}: region {r}"); same(shaded, frame[y0:y0 + h, x0:x0 + w], f"walk {mode}: shade of region {r}")
                sub["region"]["rect"] = list(r)
                sub["surface_plus_shade_over_region"] = round((m(sub, "surface_all_planes_and_albedo") + m(sub, "shade_with_mask")) / m(sub, "region"), 3)
                sub["region_over_frame_no_coverage"] = round(m(sub, "region") / f["median_ms"], 3)
                sub["pixels_over_frame_pixels"] = round(w * h / (W * H), 4)
                row[name] = sub
        out["walks"][mode] = row
        del rt, bare
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20); ap.add_argument("--scenes", default="teapot,soup100k")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "region_render.json")); ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.launches < 20:
        print("at least 20 launches", file=sys.stderr); return 2
    if a.child:
        print("RESULT " + json.dumps(measure(a.child, a.launches)), flush=True)
        return 0
    results = []
    for scene in a.scenes.split(","):
        if scene not in SCENES:
            print(f"unknown scene {scene}", file=sys.stderr); return 2
        try:                                    # a fresh process per scene, under its own time limit; nothing more is started after a failure
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", scene, "--launches", str(a.launches)], capture_output=True, text=True, timeout=SCENES[scene])
        except subprocess.TimeoutExpired:
            print(f"{scene}: no result within {SCENES[scene]} s; stopping", file=sys.stderr); return 124
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(f"{scene}: exit status {r.returncode}; stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr); return r.returncode or 1
        results.append(json.loads(line[0][7:])); print(json.dumps(results[-1]), flush=True)
    json.dump(results, open(a.out, "w"), indent=1)
    print(f"wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
