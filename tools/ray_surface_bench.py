"""Developer tool: what the per-ray surface query costs (rrt_surface_rays_device) beside the path a caller had before it, on rays that do not start at the eye.
Per scene, per ray set and per forced walk variant, on rays that are built on the device once and are the same for every timing:
  HIP-event kernel_ms, as the median of --launches alternating launches after warm-up with the relative spread (max - min) / median, of
    (a) surface_rays_into writing all twelve arrays;  (b) everything but `lights` (no shadow walk);  (c) hit / t / tri only (no attribute load);
    (d) intersect_rays_into writing hit / t / tri -- what (c) is read against;
    (e) the composed path: intersect_rays_into (hit, t), then per point light one occluded_into on the shadow rays of the hits, formed by torch on the device
        from t and the surface origin (next_origin: the composed path has no normal of its own, which is the gap the fused call closes); the forming is timed
        separately with torch events; the mask put together from (e) is compared with the fused call's bit for bit.
  The expectation that is recorded, not enforced: (a) takes no longer than the kernels of (e) together; (c) stays within the spread of (d).
Ray sets:  "reflection" = next_origin / next_dir of every hit sub-sample of the 1920 x 1080 frame;  "random" = 2^20 rays as tools/random_rays_probe.py draws them.
Scenes: the teapot and the 100 k-triangle soup.  One JSON: profiles/ray_surface.json.
   python tools/ray_surface_bench.py [--launches 20] [--scenes teapot,soup100000] [--out profiles/ray_surface.json]
Every scene is measured in a child process of its own under `timeout -k 10`; the first failure stops the run."""
import argparse, importlib, json, os, statistics, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 1920, 1080
SCENES = {"teapot": 300, "soup100000": 420}      # time limit of the child, seconds
WARMUP = 3
KINDS = ("fused_all", "fused_no_lights", "fused_hit_t_tri", "intersect_hit_t_tri", "composed_intersect", "composed_occluded")
VECTORS = ("point", "normal", "next_origin", "next_dir")


def device_arrays(torch, rrt, n, names):
    kinds = {"uint8": torch.uint8, "float64": torch.float64, "uint32": torch.int32}
    import numpy as np
    return {name: torch.empty(n * (3 if name in VECTORS else 1), dtype=kinds[np.dtype(rrt._PLANES_OF[rrt.CRaySurface][name][0]).name], device="cuda") for name in names}


def reflection_rays(torch, rrt, rt):
    """next_origin / next_dir of every hit sub-sample of the frame, from the fused call on the frame's primary rays (formed on the device)."""
    cam = rt.camera()
    f64 = dict(dtype=torch.float64, device="cuda")
    x = torch.arange(W, **f64) - (W // 2); y = (H - H // 2) - torch.arange(1, H, **f64)       # (canvas row 0 is never traced)
    a = torch.stack([x, x + 0.5, x, x + 0.5], -1) * (1.0 / W)                   # [cols][4]
    b = torch.stack([y, y, y + 0.5, y + 0.5], -1) * (1.0 / H)                   # [rows][4]
    R, U, F = (torch.tensor(cam[k], **f64) for k in ("right", "up", "forward"))
    d = ((R * a[None, :, :, None] + U * b[:, None, :, None]) + F * 1.0).reshape(-1, 3).contiguous()
    o = torch.tensor(cam["eye"], **f64).expand_as(d).contiguous()
    n = d.shape[0]
    out = device_arrays(torch, rrt, n, ("hit", "next_origin", "next_dir"))
    rt.surface_rays_into(o.reshape(-1), d.reshape(-1), out)
    seen = out["hit"].bool()
    ro, rd = out["next_origin"].reshape(-1, 3)[seen].contiguous(), out["next_dir"].reshape(-1, 3)[seen].contiguous()
    torch.cuda.synchronize()
    return ro, rd


def random_rays(torch, np, n=1 << 20):
    rng = np.random.default_rng(5)
    o = rng.uniform([-5, 0, -8], [5, 6, 5], (n, 3)); d = rng.normal(size=(n, 3))
    return torch.tensor(o, device="cuda"), torch.tensor(d, device="cuda")


def measure(scene, launches):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    rrt = importlib.import_module("rust-ray-tracer_amd"); syn = importlib.import_module("rust-ray-tracer_amd.synthetic")
    A = os.path.join(ROOT, "assets")
    sd = rrt.parse_obj_file(os.path.join(A, "model2.obj") if scene == "teapot" else syn.ensure_soup(A, 100000, syn.SEED_100K))
    lights = rrt.default_lights()
    point_lights = [(k, l) for k, l in enumerate(lights) if l.kind == 1]
    always = sum(1 << k for k, l in enumerate(lights) if l.kind != 1)
    rts = {mode: rrt.RayTracer(sd, lights, box_filter=mode) for mode in ("lane", "bundle", "ray")}
    out = dict(scene=scene, launches=launches, triangles=sd.info["n_tris"], point_lights=len(point_lights), ray_sets={})
    for name, (o, d) in (("reflection", reflection_rays(torch, rrt, rts["lane"])), ("random", random_rays(torch, np))):
        n = o.shape[0]
        o1, d1 = o.reshape(-1), d.reshape(-1)
        names = tuple(rrt.RAY_SURFACE_PLANES)
        twelve = device_arrays(torch, rrt, n, names)
        three = {k: twelve[k] for k in ("hit", "t", "tri")}
        own = device_arrays(torch, rrt, n, ("hit", "t", "tri"))               # the composed path's own outputs
        rows = {}
        for mode, rt in rts.items():
            # the composed path's shadow rays, formed once per mode (same values each time) and timed with torch events
            def form():
                seen = own["hit"].bool()
                p = o[seen] + d[seen] * own["t"][seen][:, None]
                so = twelve["next_origin"].reshape(-1, 3)[seen].contiguous()
                rays = []
                for _, l in point_lights:
                    dirv = (torch.tensor([l.v.x, l.v.y, l.v.z], dtype=torch.float64, device="cuda") - p).contiguous()
                    rays.append((dirv, torch.sqrt(dirv[:, 0] * dirv[:, 0] + dirv[:, 1] * dirv[:, 1] + dirv[:, 2] * dirv[:, 2]).contiguous()))
                return seen, so, rays
            rt.surface_rays_into(o1, d1, twelve); rt.intersect_rays_into(o1, d1, {k: own[k] for k in ("hit", "t")}); torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            form_ms = []
            for _ in range(3):
                e0.record(); seen, so, rays = form(); e1.record(); torch.cuda.synchronize(); form_ms.append(e0.elapsed_time(e1))
            m_hits = int(seen.sum())
            occ = [torch.empty(m_hits, dtype=torch.uint8, device="cuda") for _ in rays]
            ms = {k: [] for k in KINDS}

            def timed(kind, call):
                call(); ms[kind].append(rt.last_stats()["kernel_ms"])              # (waits for the launch's own events)

            def composed_occluded():
                total = 0.0
                for (dirv, mx), oc in zip(rays, occ):
                    rt.occluded_into(so.reshape(-1), dirv.reshape(-1), oc, mx); total += rt.last_stats()["kernel_ms"]
                ms["composed_occluded"].append(total)
            for i in range(WARMUP + launches):                                  # alternating: one launch of each kind per round
                timed("fused_all", lambda: rt.surface_rays_into(o1, d1, twelve))
                timed("fused_no_lights", lambda: rt.surface_rays_into(o1, d1, {k: v for k, v in twelve.items() if k != "lights"}))
                timed("fused_hit_t_tri", lambda: rt.surface_rays_into(o1, d1, three))
                timed("intersect_hit_t_tri", lambda: rt.intersect_rays_into(o1, d1, three))
                timed("composed_intersect", lambda: rt.intersect_rays_into(o1, d1, {k: own[k] for k in ("hit", "t")}))
                composed_occluded()
                if i < WARMUP:
                    for v in ms.values(): v.clear()
            rt.surface_rays_into(o1, d1, twelve); torch.cuda.synchronize()
            mask = torch.full((m_hits,), always, dtype=torch.int32, device="cuda")
            for (k, _), oc in zip(point_lights, occ):
                mask |= (1 - oc.to(torch.int32)) << k
            masks_equal = bool((mask == twelve["lights"][seen]).all()) and bool((twelve["lights"][~seen] == 0).all())
            assert masks_equal, (scene, name, mode)                             # faster and different is not faster
            med = {k: statistics.median(v) for k, v in ms.items()}
            spread = {k: (max(v) - min(v)) / med[k] for k, v in ms.items()}
            row = {f"{k}_kernel_ms": round(med[k], 4) for k in KINDS}
            row.update({f"{k}_relative_spread": round(spread[k], 4) for k in KINDS})
            composed = med["composed_intersect"] + med["composed_occluded"]
            row["composed_kernels_ms"] = round(composed, 4)
            row["composed_forming_torch_ms"] = round(statistics.median(form_ms), 4)
            row["fused_all_over_composed_kernels"] = round(med["fused_all"] / composed, 3)
            row["fused_all_no_longer_than_composed_kernels"] = bool(med["fused_all"] <= composed)
            row["fused_hit_t_tri_over_intersect"] = round(med["fused_hit_t_tri"] / med["intersect_hit_t_tri"], 3)
            row["fused_hit_t_tri_within_spread_of_intersect"] = bool(abs(med["fused_hit_t_tri"] - med["intersect_hit_t_tri"]) <= spread["intersect_hit_t_tri"] * med["intersect_hit_t_tri"])
            row["masks_equal_bit_for_bit"] = masks_equal
            rows[mode] = row
            del seen, so, rays, occ, mask
        out["ray_sets"][name] = dict(rays=n, hit_fraction=round(float(twelve["hit"].float().mean()), 4), walks=rows)
        del twelve, own, o, d
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20); ap.add_argument("--scenes", default="teapot,soup100000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ray_surface.json")); ap.add_argument("--child", default=None)
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
