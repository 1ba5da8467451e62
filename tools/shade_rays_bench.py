"""Developer tool: what shading a ray batch from its kept records costs (rrt_shade_rays_device) beside the path a caller had before it, rrt_get_ray_colours_device
on the same rays, which walks every first hit and every shadow ray again.
Per scene, per ray set and per forced walk variant, on rays and records that are built on the device once and are the same for every timing:
  HIP-event kernel_ms, as the median of --launches alternating launches after warm-up with the relative spread (max - min) / median, of
    (a) shade_rays_into writing colour from the records with their mask;  (b) the same without the mask (the shadow rays of the records' hits are walked);
    (c) local + kr only, with the mask (no walk at all);  (d) get_ray_colours_into on the same rays: existing code, the baseline.
  The colours of (a) and (b) are compared with (d)'s bit for bit, and (c) with the local / kr of a launch that writes all three.
  The expectation that is recorded, not enforced: (a) takes no longer than (d), and far less where nothing reflects (the soup has no mirror).
Ray sets:  "reflection" = next_origin / next_dir of every hit sub-sample of the 1920 x 1080 frame;  "random" = 2^20 rays as tools/random_rays_probe.py draws them
(the sets of tools/ray_surface_bench.py).  Scenes: the teapot and the 100 k-triangle soup.  One JSON: profiles/shade_rays.json.
   python tools/shade_rays_bench.py [--launches 20] [--scenes teapot,soup100000] [--out profiles/shade_rays.json]
Every scene is measured in a child process of its own under `timeout -k 10`; the first failure stops the run."""
import argparse, importlib, json, os, statistics, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ray_surface_bench import device_arrays, random_rays, reflection_rays

SCENES = {"teapot": 300, "soup100000": 420}      # time limit of the child, seconds
WARMUP = 3
KINDS = ("shade_mask", "shade_no_mask", "local_kr_mask", "get_ray_colours")
RECORDS = ("albedo", "point", "normal", "material", "lights")


def measure(scene, launches):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    rrt = importlib.import_module("rust-ray-tracer_amd"); syn = importlib.import_module("rust-ray-tracer_amd.synthetic")
    A = os.path.join(ROOT, "assets")
    sd = rrt.parse_obj_file(os.path.join(A, "model2.obj") if scene == "teapot" else syn.ensure_soup(A, 100000, syn.SEED_100K))
    lights = rrt.default_lights()
    kr_table = torch.tensor([float(m["kr"]) for m in sd.materials()] + [0.0], device="cuda")
    rts = {mode: rrt.RayTracer(sd, lights, box_filter=mode) for mode in ("lane", "bundle", "ray")}
    out = dict(scene=scene, launches=launches, triangles=sd.info["n_tris"], lights=len(lights), ray_sets={})
    for name, (o, d) in (("reflection", reflection_rays(torch, rrt, rts["lane"])), ("random", random_rays(torch, np))):
        n = o.shape[0]
        o1, d1 = o.reshape(-1), d.reshape(-1)
        rec = device_arrays(torch, rrt, n, RECORDS + ("hit",))
        rts["lane"].surface_rays_into(o1, d1, rec); torch.cuda.synchronize()            # (the records are the same in every walk: tests/test_gpu_ray_surface.py)
        hit = rec.pop("hit").bool()
        material = (rec["material"].to(torch.int64) & 0xFFFFFFFF).clamp(max=len(kr_table) - 1)
        mirror_fraction = float((hit & (kr_table[material] > 0.0)).float().mean())
        no_mask = {k: v for k, v in rec.items() if k != "lights"}
        colour = {k: torch.empty(n, dtype=torch.int32, device="cuda") for k in ("mask", "no_mask", "all", "old")}
        local, kr, local2, kr2 = (torch.empty(n * w, dtype=torch.float64, device="cuda") for w in (3, 1, 3, 1))
        rows = {}
        for mode, rt in rts.items():
            ms = {k: [] for k in KINDS}

            def timed(kind, call):
                call(); ms[kind].append(rt.last_stats()["kernel_ms"])                  # (waits for the launch's own events)
            for i in range(WARMUP + launches):                                          # alternating: one launch of each kind per round
                timed("shade_mask", lambda: rt.shade_rays_into({"colour": colour["mask"]}, d1, rec))
                timed("shade_no_mask", lambda: rt.shade_rays_into({"colour": colour["no_mask"]}, d1, no_mask))
                timed("local_kr_mask", lambda: rt.shade_rays_into({"local": local, "kr": kr}, d1, rec))
                timed("get_ray_colours", lambda: rt.get_ray_colours_into(o1, d1, colour["old"]))
                if i < WARMUP:
                    for v in ms.values(): v.clear()
            rt.shade_rays_into({"colour": colour["all"], "local": local2, "kr": kr2}, d1, rec); torch.cuda.synchronize()
            equal = all(bool((colour[k] == colour["old"]).all()) for k in ("mask", "no_mask", "all"))
            equal = equal and bool((local.view(torch.int64) == local2.view(torch.int64)).all()) and bool((kr.view(torch.int64) == kr2.view(torch.int64)).all())
            assert equal, (scene, name, mode)                                           # faster and different is not faster
            med = {k: statistics.median(v) for k, v in ms.items()}
            spread = {k: (max(v) - min(v)) / med[k] for k, v in ms.items()}
            row = {f"{k}_kernel_ms": round(med[k], 4) for k in KINDS}
            row.update({f"{k}_relative_spread": round(spread[k], 4) for k in KINDS})
            for k in KINDS[:3]:
                row[f"{k}_over_get_ray_colours"] = round(med[k] / med["get_ray_colours"], 3)
            row["shade_mask_no_longer_than_get_ray_colours"] = bool(med["shade_mask"] <= med["get_ray_colours"])
            row["colours_equal_bit_for_bit"] = equal
            rows[mode] = row
        out["ray_sets"][name] = dict(rays=n, hit_fraction=round(float(hit.float().mean()), 4), mirror_fraction=round(mirror_fraction, 4), walks=rows)
        del rec, no_mask, colour, local, kr, local2, kr2, o, d
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20); ap.add_argument("--scenes", default="teapot,soup100000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shade_rays.json")); ap.add_argument("--child", default=None)
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
        # a fresh process per scene under its own time limit; nothing more is started after a failure
        r = subprocess.run(["timeout", "-k", "10", str(SCENES[scene]), sys.executable, os.path.abspath(__file__), "--child", scene, "--launches", str(a.launches)],
                           capture_output=True, text=True)
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(f"{scene}: exit status {r.returncode}; stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr); return r.returncode or 1
        results.append(json.loads(line[0][7:])); print(json.dumps(results[-1]), flush=True)
    json.dump(results, open(a.out, "w"), indent=1)
    print(f"wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
