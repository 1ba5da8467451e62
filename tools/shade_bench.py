"""Developer tool: what shading a frame from its kept surface buffers costs (rrt_shade_surface_device) beside the launch that writes the buffers and beside the
frame itself.  Per scene and per forced walk variant, HIP-event kernel_ms as the median of --launches launches after warm-up, with the spread (min, max),
measured in this order:
  (1) rrt_render_surface_device with all four surface planes and the albedo plane: what a host keeps in order to shade;
  (2) rrt_shade_surface_device of those planes, the mask of lit lights included: no depth-0 shadow ray is walked;
  (3) rrt_shade_surface_device without the mask: the depth-0 shadow rays are walked again;
  (4) rrt_render_visibility_device with the t and tri planes: the primary walk alone;
  (5) rrt_render_device of the same frame.
The shaded frames of (2) and (3) are compared with the frame of (5); a difference fails the run.
Scenes: the teapot and the 100 k-triangle soup, both at 1920 x 1080 in the creation pose.  One JSON: profiles/shade.json.
   python tools/shade_bench.py [--launches 20] [--scenes teapot,soup100k] [--out profiles/shade.json]
Every scene is measured in a child process of its own under a time limit; the first failure stops the run."""
import argparse, importlib, json, os, statistics, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 1920, 1080
SCENES = {"teapot": 300, "soup100k": 420}       # time limit of the child, seconds
WARMUP = 3


def measure(scene, launches):
    import torch
    sys.path.insert(0, ROOT)
    rrt = importlib.import_module("rust-ray-tracer_amd"); syn = importlib.import_module("rust-ray-tracer_amd.synthetic")
    A = os.path.join(ROOT, "assets")
    sd = rrt.parse_obj_file(os.path.join(A, "model2.obj") if scene == "teapot" else syn.ensure_soup(A, 100000, syn.SEED_100K))
    planes = dict(point=torch.empty((H, W, 4, 3), dtype=torch.float64, device="cuda"), normal=torch.empty((H, W, 4, 3), dtype=torch.float64, device="cuda"),
                  material=torch.empty((H, W, 4), dtype=torch.int32, device="cuda"), lights=torch.empty((H, W, 4), dtype=torch.int32, device="cuda"),
                  albedo=torch.empty((H, W, 4), dtype=torch.int32, device="cuda"))
    no_mask = {n: t for n, t in planes.items() if n != "lights"}
    primary = dict(t=torch.empty((H, W, 4), dtype=torch.float64, device="cuda"), tri=torch.empty((H, W, 4), dtype=torch.int32, device="cuda"))
    fb, shaded = (torch.empty((H, W), dtype=torch.int32, device="cuda") for _ in range(2))

    def timed(rt, launch):
        ms = []
        for i in range(WARMUP + launches):
            launch(); torch.cuda.synchronize()
            if i >= WARMUP: ms.append(rt.last_stats()["kernel_ms"])
        return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4))

    out = dict(scene=scene, size=f"{W}x{H}", launches=launches, triangles=sd.info["n_tris"], walks={})
    for mode in ("lane", "bundle", "ray"):
        rt = rrt.RayTracer(sd, rrt.default_lights(), box_filter=mode)
        row = dict(surface_all_planes_and_albedo=timed(rt, lambda: rt.surface_into(planes, W, H)))
        row["shade_with_mask"] = timed(rt, lambda: rt.shade_into(shaded, planes, W, H))
        with_mask = shaded.clone()
        row["shade_without_mask"] = timed(rt, lambda: rt.shade_into(shaded, no_mask, W, H))
        row["visibility_t_tri"] = timed(rt, lambda: rt.visibility_into(primary, W, H))
        row["frame"] = timed(rt, lambda: rt.render_into(fb, W, H))
        if not (torch.equal(with_mask, fb) and torch.equal(shaded, fb)):
            raise SystemExit(f"{scene}, walk {mode}: a shaded frame differs from the rendered frame")
        material = planes["material"].cpu().numpy().view("uint32")
        row["rays_hit_fraction"] = round(float((material != 0xFFFFFFFF).mean()), 4)
        m = lambda k: row[k]["median_ms"]
        row["shade_with_mask_over_frame"] = round(m("shade_with_mask") / m("frame"), 3)
        row["shade_without_mask_over_frame"] = round(m("shade_without_mask") / m("frame"), 3)
        row["shade_without_mask_over_frame_minus_primary_walk"] = round(m("shade_without_mask") / (m("frame") - m("visibility_t_tri")), 3)
        row["surface_plus_shade_with_mask_over_frame"] = round((m("surface_all_planes_and_albedo") + m("shade_with_mask")) / m("frame"), 3)
        out["walks"][mode] = row
        del rt
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20); ap.add_argument("--scenes", default="teapot,soup100k")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shade.json")); ap.add_argument("--child", default=None)
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
