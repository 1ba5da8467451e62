"""Developer tool: what on-device tile selection (rrt_mark_tiles_device, rrt_select_tiles_device) costs, and what a frame repaired through its list costs beside
the whole frame.  HIP-event times as the median of --launches launches after warm-up, with the spread (min, max).
  (a) the mark launch per plane kind -- the uint32 `material` plane and the uint8 `hit` plane of a surface / visibility launch (SET, NONZERO), two framebuffers
      (DIFFERS), two `t` planes (DIFFERS over doubles) -- with the bytes it reads and the achieved bytes/s, beside the compaction launch's figure in
      profiles/compact.json (the project's own bandwidth yardstick); the whole selection (marks + compaction); and the path a caller had, restated in torch on the
      device: pad, reshape, any, nonzero (which synchronises).  The two lists must be equal.
  (b) the material edit at full size: rrt_raytracer_set_materials of material 0, then select (SET {0, every mirror}) + rrt_render_tile_list_device into the old
      frame, against rrt_render_device of the whole frame, per forced walk.  Every repaired frame is compared bit for bit with the whole one.
Scenes: the teapot and the 100 k-triangle soup, both at 1920 x 1080 in the creation pose.  One JSON: profiles/tile_select.json.
   python tools/tile_select_bench.py [--launches 20] [--scenes teapot,soup100k] [--out profiles/tile_select.json]
Every scene is measured in a child process of its own under a time limit; the first failure stops the run."""
import argparse, importlib, json, os, statistics, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 1920, 1080
SCENES = {"teapot": 300, "soup100k": 420}       # time limit of the child, seconds
WARMUP = 3


def measure(scene, launches):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    rrt = importlib.import_module("rust-ray-tracer_amd"); syn = importlib.import_module("rust-ray-tracer_amd.synthetic")
    A = os.path.join(ROOT, "assets")
    sd = rrt.parse_obj_file(os.path.join(A, "model2.obj") if scene == "teapot" else syn.ensure_soup(A, 100000, syn.SEED_100K))
    tiles_x, tiles_y = rrt.tile_count(W, H)
    n_tiles = tiles_x * tiles_y
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device="cuda")
    marks, tiles, count = torch.empty(n_tiles, dtype=torch.uint8, device="cuda"), i32(n_tiles), i32(1)
    scratch = torch.empty(rrt.compact_scratch_bytes(n_tiles), dtype=torch.uint8, device="cuda")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(launch):
        """median / min / max of the event time around launch(), ms"""
        ms = []
        for i in range(WARMUP + launches):
            torch.cuda.synchronize()
            ev[0].record(); launch(); ev[1].record()
            torch.cuda.synchronize()
            if i >= WARMUP: ms.append(ev[0].elapsed_time(ev[1]))
        return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4))

    def by_torch(passed):
        """the list by torch on the device: [H][W](...) bool -> pad to whole tiles, reshape, any, nonzero"""
        p = passed.reshape(H, W, -1)
        padded = torch.zeros((tiles_y * 8, tiles_x * 8, p.shape[2]), dtype=torch.bool, device="cuda")
        padded[:H, :W] = p
        return torch.nonzero(padded.reshape(tiles_y, 8, tiles_x, 8, -1).any(4).any(3).any(1).reshape(-1)).reshape(-1)

    rt = rrt.RayTracer(sd, rrt.default_lights())
    mats = rt.materials()
    mirrors = [k for k, m in enumerate(mats) if m["kr"] > 0]
    material, hit, t0, t1 = i32(H, W, 4), torch.empty((H, W, 4), dtype=torch.uint8, device="cuda"), torch.empty((H, W, 4), dtype=torch.float64, device="cuda"), None
    fb0, fb1 = i32(H, W), i32(H, W)
    rt.surface_into({"material": material}, W, H); rt.visibility_into({"hit": hit, "t": t0}, W, H); rt.render_into(fb0, W, H)
    edited = [dict(m) for m in mats]
    edited[0] = dict(edited[0], kd=(0.3, 0.9, 0.5))
    rt.set_materials(edited); rt.render_into(fb1, W, H); rt.set_materials(mats)
    torch.cuda.synchronize()
    t1 = t0.clone(); t1[H // 4:H // 2, W // 4:W // 2] += 1.0        # (a `t` plane that differs in a sixteenth of the frame)
    in_set = torch.zeros(256, dtype=torch.bool, device="cuda"); in_set[[0] + mirrors] = True
    kinds = {"material_set": (rrt.tile_test("set", material, values=[0] + mirrors), material.numel() * 4,
                              lambda: material.ge(0) & material.lt(256) & in_set[material.clamp(min=0, max=255).long()]),   # (int32 bits: 0xFFFFFFFF is -1)
             "hit_nonzero": (rrt.tile_test("nonzero", hit), hit.numel(), lambda: hit != 0),
             "framebuffers_differ": (rrt.tile_test("differs", fb0, fb1), 2 * fb0.numel() * 4, lambda: fb0 != fb1),
             "t_planes_differ": (rrt.tile_test("differs", t0, t1), 2 * t0.numel() * 8, lambda: t0.view(torch.int64) != t1.view(torch.int64))}
    out = dict(scene=scene, size=f"{W}x{H}", launches=launches, triangles=sd.info["n_tris"], tiles=n_tiles, mirrors=mirrors, planes={}, edit={})
    for name, (test, read_bytes, passed) in kinds.items():
        row = dict(mark=timed(lambda: rt.mark_tiles_into(marks, test, W, H)), read_bytes=read_bytes)
        row["mark_gbytes_per_s"] = round(read_bytes / row["mark"]["median_ms"] / 1e6, 1)
        row["select"] = timed(lambda: rt.select_tiles_into(tiles, count, marks, scratch, test, W, H))
        torch.cuda.synchronize()
        n = int(count.cpu().numpy().view(np.uint32)[0])
        want = by_torch(passed())
        if not torch.equal(tiles[:n].long(), want):
            raise SystemExit(f"{scene}: {name}: the list of {n} tiles differs from torch's of {want.numel()}")
        row["tiles_selected"] = n
        row["torch_pad_reshape_any_nonzero"] = timed(lambda: by_torch(passed()))
        row["select_over_torch"] = round(row["select"]["median_ms"] / row["torch_pad_reshape_any_nonzero"]["median_ms"], 3)
        out["planes"][name] = row
    del rt
    # (b) the material edit, per forced walk
    for mode in ("lane", "bundle", "ray"):
        rt = rrt.RayTracer(sd, rrt.default_lights(), box_filter=mode, coverage=False)
        frame, repaired, old = i32(H, W), i32(H, W), i32(H, W)
        rt.surface_into({"material": material}, W, H); rt.render_into(old, W, H)
        rt.set_materials(edited)
        test = rrt.tile_test("set", material, values=[0] + mirrors)

        def repair():
            rt.select_tiles_into(tiles, count, marks, scratch, test, W, H)
            rt.render_tile_list_into(repaired, tiles, W, H, bound_t=count)
        repaired.copy_(old)
        row = dict(whole_frame=timed(lambda: rt.render_into(frame, W, H)), select_plus_tile_list=timed(repair))
        torch.cuda.synchronize()
        if not torch.equal(repaired, frame):
            raise SystemExit(f"{scene}: walk {mode}: the repaired frame differs from the whole one on {int((repaired != frame).sum())} pixels")
        row["tiles_selected"] = int(count.cpu().numpy().view(np.uint32)[0])
        row["pixels_changed"] = int((frame != old).sum())
        row["repair_over_whole_frame"] = round(row["select_plus_tile_list"]["median_ms"] / row["whole_frame"]["median_ms"], 3)
        row["repair_is_faster"] = bool(row["select_plus_tile_list"]["median_ms"] < row["whole_frame"]["median_ms"])
        out["edit"][mode] = row
        del rt
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20); ap.add_argument("--scenes", default="teapot,soup100k")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tile_select.json")); ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.launches < 20:
        print("at least 20 launches", file=sys.stderr); return 2
    if a.child:
        print("RESULT " + json.dumps(measure(a.child, a.launches)), flush=True)
        return 0
    yardstick = None
    try:
        yardstick = {r["scene"]: r["record_sets"]["level1"]["compact_gbytes_per_s"] for r in json.load(open(os.path.join(ROOT, "profiles", "compact.json")))}
    except (OSError, KeyError, ValueError):
        pass
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
        results.append(json.loads(line[0][7:]))
        if yardstick and scene in yardstick:
            results[-1]["compact_gbytes_per_s_in_profiles_compact_json"] = yardstick[scene]
        print(json.dumps(results[-1]), flush=True)
    json.dump(results, open(a.out, "w"), indent=1)
    print(f"wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
