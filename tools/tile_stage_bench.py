"""Developer tool: what the deferred stages over a device-resident tile list cost (rrt_render_visibility_tile_list_device, rrt_render_surface_tile_list_device,
rrt_shade_surface_tile_list_device, rrt_ambient_surface_tile_list_device) beside their region twins and beside the paths a caller had.  HIP-event times as the
median of --launches launches after warm-up, with the spread (min, max), per forced walk (lane / bundle / ray).  Every timed output is compared bit for bit with
the region call's.
  (a) each stage over all 32 400 tiles in ascending order, against its region twin with region == NULL.  The twin is the yardstick: `held` says whether the
      list's median lies inside the twin's own min-max.  Reported, not tuned.
  (b) each stage over a seeded quarter of the tiles.
  (c) the material edit of tools/tile_select_bench.py (kd of material 0), repaired three ways: select + rrt_render_tile_list_device; select + the shade stage
      over the list with the mask; rrt_shade_surface_device of the whole frame.
  (d) a tex / bump edit of material 0: select + surface stage + select + shade stage over the lists, against whole-frame surface + shade.
  (e) adaptive ambient occlusion: 8 directions everywhere + RANGE select + 32 directions on the selected tiles, against 32 directions everywhere, with the
      share of the tiles selected.
Scenes: the teapot and the 100 k-triangle soup, both at 1920 x 1080 in the creation pose.  One JSON: profiles/tile_stages.json.
   python tools/tile_stage_bench.py [--launches 20] [--scenes teapot,soup100k] [--out profiles/tile_stages.json]
Every scene is measured in a child process of its own under a time limit; the first failure stops the run."""
import argparse, importlib, json, math, os, statistics, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 1920, 1080
SCENES = {"teapot": 300, "soup100k": 600}       # time limit of the child, seconds
WARMUP = 3
MAX_T = 2.0
VIS = ("hit", "t", "u", "v", "tri", "albedo")
SURF = ("point", "normal", "material", "lights")


def table(n):
    """8 directions on a ring of mixed elevations; for n = 32, 24 more on a finer ring behind them (the first eight of the two tables are the same)."""
    ring = lambda m, cs: [[math.sqrt(1 - c * c) * math.cos(2 * math.pi * (k + 0.5) / m), math.sqrt(1 - c * c) * math.sin(2 * math.pi * (k + 0.5) / m), c]
                          for k in range(m) for c in [cs[k % len(cs)]]]
    return ring(8, (0.3, 0.6, 0.85, 0.45)) + (ring(24, (0.2, 0.5, 0.7, 0.9, 0.35, 0.8)) if n == 32 else [])


def measure(scene, launches):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    rrt = importlib.import_module("rust-ray-tracer_amd"); syn = importlib.import_module("rust-ray-tracer_amd.synthetic")
    A = os.path.join(ROOT, "assets")
    sd = rrt.parse_obj_file(os.path.join(A, "model2.obj") if scene == "teapot" else syn.ensure_soup(A, 100000, syn.SEED_100K))
    tiles_x, tiles_y = rrt.tile_count(W, H)
    n_tiles = tiles_x * tiles_y
    kinds = dict(hit=torch.uint8, t=torch.float64, u=torch.float64, v=torch.float64, point=torch.float64, normal=torch.float64)
    shape = lambda name: (H, W, 4, 3) if name in ("point", "normal") else (H, W) if name in ("fb", "grey") else (H, W, 4)
    new = lambda name, fill=0: torch.full(shape(name), fill, dtype=kinds.get(name, torch.int32), device="cuda")
    planes_of = lambda names, fill=0: {n: new(n, fill) for n in names}
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device="cuda")
    marks, scratch = torch.empty(n_tiles, dtype=torch.uint8, device="cuda"), torch.empty(rrt.compact_scratch_bytes(n_tiles), dtype=torch.uint8, device="cuda")
    every = torch.arange(n_tiles, dtype=torch.int32, device="cuda")
    quarter = torch.from_numpy(np.random.default_rng(5).permutation(n_tiles)[:n_tiles // 4].astype(np.int32)).cuda()
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

    def bits(t):
        return t.view(torch.int64) if t.dtype == torch.float64 else t

    def pixels_of(tiles):
        """[H][W] bool on the device: the pixels inside the listed tiles"""
        m = torch.zeros(n_tiles, dtype=torch.bool, device="cuda"); m[tiles.long()] = True
        return m.reshape(tiles_y, tiles_x).repeat_interleave(8, 0).repeat_interleave(8, 1)[:H, :W]

    def same(got, want, mask, what):
        for n in got:
            g, w = bits(got[n]), bits(want[n])
            k = mask.reshape(mask.shape + (1,) * (g.dim() - 2))
            if not torch.equal(torch.where(k, g, torch.zeros_like(g)), torch.where(k, w, torch.zeros_like(w))):
                raise SystemExit(f"{scene}: {what}: plane {n} differs from the region call's inside the listed tiles")

    def selected(count):
        return int(count.cpu().numpy().view(np.uint32)[0])

    out = dict(scene=scene, size=f"{W}x{H}", launches=launches, triangles=sd.info["n_tris"], tiles=n_tiles, walks={})
    for mode in ("lane", "bundle", "ray"):
        rt = rrt.RayTracer(sd, rrt.default_lights(), box_filter=mode, coverage=False)
        mats = rt.materials()
        mirrors = [k for k, m in enumerate(mats) if m["kr"] > 0]
        ten, fb, amb = planes_of(VIS + SURF), new("fb"), planes_of(("occluded", "grey"))
        t8, t32 = table(8), table(32)
        # the region twins, and what they write: the references of everything below
        twins = {"visibility": lambda: rt.visibility_into({n: ten[n] for n in VIS}, W, H), "surface": lambda: rt.surface_into(ten, W, H),
                 "shade": lambda: rt.shade_into(fb, ten, W, H), "ambient": lambda: rt.ambient_into(amb, ten, t32, MAX_T, W, H)}
        row = dict(all_tiles={}, quarter={})
        twin_ms = {stage: timed(launch) for stage, launch in twins.items()}
        want = {"visibility": {n: ten[n] for n in VIS}, "surface": ten, "shade": {"fb": fb}, "ambient": amb}
        for part, tiles in (("all_tiles", every), ("quarter", quarter)):
            got = {"visibility": planes_of(VIS, 0x25), "surface": planes_of(VIS + SURF, 0x25), "shade": {"fb": new("fb", 0x25)}, "ambient": planes_of(("occluded", "grey"), 0x25)}
            lists = {"visibility": lambda: rt.visibility_tile_list_into(got["visibility"], tiles, W, H), "surface": lambda: rt.surface_tile_list_into(got["surface"], tiles, W, H),
                     "shade": lambda: rt.shade_tile_list_into(got["shade"]["fb"], ten, tiles, W, H),
                     "ambient": lambda: rt.ambient_tile_list_into(got["ambient"], ten, t32, MAX_T, tiles, W, H)}
            mask = pixels_of(tiles)
            for stage, launch in lists.items():
                r = dict(tile_list=timed(launch))
                same(got[stage], want[stage], mask, f"walk {mode}: {stage} over {part}")
                if part == "all_tiles":
                    r["region_twin"] = twin_ms[stage]
                    r["list_over_twin"] = round(r["tile_list"]["median_ms"] / twin_ms[stage]["median_ms"], 3)
                    r["held"] = bool(twin_ms[stage]["min_ms"] <= r["tile_list"]["median_ms"] <= twin_ms[stage]["max_ms"])
                else:
                    r["list_over_whole_frame_twin"] = round(r["tile_list"]["median_ms"] / twin_ms[stage]["median_ms"], 3)
                row[part][stage] = r
            del got
        # (c) the material edit: kd of material 0; the kept planes stay valid
        tiles, count, frame, repaired = i32(n_tiles), i32(1), new("fb"), new("fb")
        whole = timed(lambda: rt.render_into(frame, W, H))
        old = frame.clone()
        edited = [dict(m) for m in mats]
        edited[0] = dict(edited[0], kd=(0.3, 0.9, 0.5))
        rt.set_materials(edited)
        rt.render_into(frame, W, H)
        test = rrt.tile_test("set", ten["material"], values=[0] + mirrors)
        edit = dict(whole_frame_render=whole)

        def by_render():
            rt.select_tiles_into(tiles, count, marks, scratch, test, W, H)
            rt.render_tile_list_into(repaired, tiles, W, H, bound_t=count)

        def by_shade():
            rt.select_tiles_into(tiles, count, marks, scratch, test, W, H)
            rt.shade_tile_list_into(repaired, ten, tiles, W, H, bound_t=count)
        for name, launch in (("select_plus_render_tile_list", by_render), ("select_plus_shade_tile_list", by_shade), ("whole_frame_shade", lambda: rt.shade_into(repaired, ten, W, H))):
            repaired.copy_(old)
            edit[name] = timed(launch)
            torch.cuda.synchronize()
            if not torch.equal(repaired, frame):
                raise SystemExit(f"{scene}: walk {mode}: {name}: the repaired frame differs from the whole one on {int((repaired != frame).sum())} pixels")
            edit[name + "_over_frame"] = round(edit[name]["median_ms"] / whole["median_ms"], 3)
        edit["tiles_selected"], edit["pixels_changed"] = selected(count), int((frame != old).sum())
        row["material_edit"] = edit
        # (d) the tex / bump edit of material 0: the kept albedo and normal planes are stale under it
        donor = next((k for k, m in enumerate(mats) if (m["tex"], m["bump"]) != (mats[0]["tex"], mats[0]["bump"]) and m["bump"] >= 0), None)
        if donor is None:
            row["tex_edit"] = "no material with another tex and bump"
        else:
            edited[0] = dict(edited[0], tex=mats[donor]["tex"], bump=mats[donor]["bump"])
            rt.set_materials(edited)
            fresh, fresh_fb = planes_of(VIS + SURF), new("fb")
            tex = dict(whole_frame_surface=timed(lambda: rt.surface_into(fresh, W, H)), whole_frame_shade=timed(lambda: rt.shade_into(fresh_fb, fresh, W, H)))
            rt.render_into(frame, W, H)
            tiles_b, count_b = i32(n_tiles), i32(1)
            test_a = rrt.tile_test("set", ten["material"], values=[0])

            def repair():
                rt.select_tiles_into(tiles, count, marks, scratch, test_a, W, H)
                rt.select_tiles_into(tiles_b, count_b, marks, scratch, test, W, H)
                rt.surface_tile_list_into(ten, tiles, W, H, bound_t=count)
                rt.shade_tile_list_into(repaired, ten, tiles_b, W, H, bound_t=count_b)
            tex["two_selects_plus_surface_and_shade_tile_lists"] = timed(repair)
            torch.cuda.synchronize()
            if not torch.equal(repaired, frame) or not torch.equal(fresh_fb, frame):
                raise SystemExit(f"{scene}: walk {mode}: the frame repaired after the tex edit differs from the whole one")
            same(ten, fresh, pixels_of(every), f"walk {mode}: the planes repaired after the tex edit")
            both = tex["whole_frame_surface"]["median_ms"] + tex["whole_frame_shade"]["median_ms"]
            tex["repair_over_whole_frame_surface_plus_shade"] = round(tex["two_selects_plus_surface_and_shade_tile_lists"]["median_ms"] / both, 3)
            tex["tiles_surface"], tex["tiles_shade"], tex["donor_material"] = selected(count), selected(count_b), donor
            row["tex_edit"] = tex
            del fresh
        # (e) adaptive ambient occlusion
        occ8, occ32, ref32 = new("occluded"), new("occluded"), new("occluded")
        test8 = rrt.tile_test("range", occ8, lo=1, hi=255)

        def adaptive():
            rt.ambient_into({"occluded": occ8}, ten, t8, MAX_T, W, H)
            rt.select_tiles_into(tiles, count, marks, scratch, test8, W, H)
            rt.ambient_tile_list_into({"occluded": occ32}, ten, t32, MAX_T, tiles, W, H, bound_t=count)
        ao = dict(n32_everywhere=timed(lambda: rt.ambient_into({"occluded": ref32}, ten, t32, MAX_T, W, H)), n8_everywhere_select_n32_on_the_list=timed(adaptive))
        torch.cuda.synchronize()
        n = selected(count)
        same({"occluded": occ32}, {"occluded": ref32}, pixels_of(tiles[:n]), f"walk {mode}: adaptive ambient occlusion")
        ao["tiles_selected"], ao["share_selected"] = n, round(n / n_tiles, 3)
        ao["adaptive_over_n32_everywhere"] = round(ao["n8_everywhere_select_n32_on_the_list"]["median_ms"] / ao["n32_everywhere"]["median_ms"], 3)
        row["adaptive_ambient"] = ao
        out["walks"][mode] = row
        del rt, ten
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20); ap.add_argument("--scenes", default="teapot,soup100k")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tile_stages.json")); ap.add_argument("--child", default=None)
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
        results.append(json.loads(line[0][7:]))
        print(json.dumps(results[-1]), flush=True)
    json.dump(results, open(a.out, "w"), indent=1)
    print(f"wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
