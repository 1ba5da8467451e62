"""Developer tool: what the device-resident ray batches cost (rrt_occluded_rays_device, rrt_intersect_rays_device) beside each other and beside the host form.
Per scene, per ray set and per forced walk variant, on rays that are built on the device once and are the same for every timing:
  HIP-event kernel_ms, as the median of --launches alternating launches after warm-up, of
    (a) occluded_into;  (b) intersect_rays_into with all five planes;  (c) intersect_rays_into with `hit` only;
  the minimum and maximum of each and the relative spread (max - min) / median of (b), the repeated kernel the ratios are read against;
  wall time of the host form intersect_rays (two or three uploads, five downloads) against intersect_rays_into + torch.cuda.synchronize().
Ray sets:  "shadow" = for every sub-sample of the 1920 x 1080 frame that hits (the hit and t planes of visibility_into), the ray from the hit point, moved 1e-4
along -d/|d|, towards the first point light of default_lights(), max_t = |direction|;  "random" = 2^20 rays as tools/random_rays_probe.py draws them, max_t = None.
Scenes: the teapot and the 100 k-triangle soup.  One JSON: profiles/ray_batches.json.
   python tools/ray_batch_bench.py [--launches 20] [--scenes teapot,soup100000] [--out profiles/ray_batches.json]
Every scene is measured in a child process of its own under `timeout -k 10`; the first failure stops the run."""
import argparse, importlib, json, os, statistics, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 1920, 1080
SCENES = {"teapot": 300, "soup100000": 420}      # time limit of the child, seconds
WARMUP = 3
HOST_REPS = 3
KINDS = ("occluded", "intersect_all", "intersect_hit_only")


def shadow_rays(torch, rrt, rt):
    """Shadow-shaped rays of every hit sub-sample of the frame, formed on the device from the visibility planes."""
    planes = dict(hit=torch.empty((H, W, 4), dtype=torch.uint8, device="cuda"), t=torch.empty((H, W, 4), dtype=torch.float64, device="cuda"))
    rt.visibility_into(planes, W, H)
    cam = rt.camera()
    f64 = dict(dtype=torch.float64, device="cuda")
    x = torch.arange(W, **f64) - (W // 2); y = (H - H // 2) - torch.arange(H, **f64)
    a = torch.stack([x, x + 0.5, x, x + 0.5], -1) * (1.0 / W)                   # [cols][4]
    b = torch.stack([y, y, y + 0.5, y + 0.5], -1) * (1.0 / H)                   # [rows][4]
    R, U, F = (torch.tensor(cam[k], **f64) for k in ("right", "up", "forward"))
    d = (R * a[None, :, :, None] + U * b[:, None, :, None]) + F * 1.0           # [rows][cols][4][3]
    seen = planes["hit"].bool()
    d = d[seen]; t = planes["t"][seen]
    light = next(l for l in rrt.default_lights() if l.kind == 1)
    p = torch.tensor(cam["eye"], **f64) + d * t[:, None]
    ro = (p - d / torch.linalg.norm(d, dim=1, keepdim=True) * 1e-4).contiguous()
    dirv = (torch.tensor([light.v.x, light.v.y, light.v.z], **f64) - ro).contiguous()
    max_t = torch.linalg.norm(dirv, dim=1).contiguous()
    torch.cuda.synchronize()
    return ro, dirv, max_t


def random_rays(torch, np, n=1 << 20):
    rng = np.random.default_rng(5)
    o = rng.uniform([-5, 0, -8], [5, 6, 5], (n, 3)); d = rng.normal(size=(n, 3))
    return torch.tensor(o, device="cuda"), torch.tensor(d, device="cuda"), None


def measure(scene, launches):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    rrt = importlib.import_module("rust-ray-tracer_amd"); syn = importlib.import_module("rust-ray-tracer_amd.synthetic")
    A = os.path.join(ROOT, "assets")
    sd = parse = rrt.parse_obj_file(os.path.join(A, "model2.obj") if scene == "teapot" else syn.ensure_soup(A, 100000, syn.SEED_100K))
    rts = {mode: rrt.RayTracer(sd, rrt.default_lights(), box_filter=mode) for mode in ("lane", "bundle", "ray")}
    out = dict(scene=scene, launches=launches, triangles=sd.info["n_tris"], ray_sets={})
    for name, (o, d, m) in (("shadow", shadow_rays(torch, rrt, rts["lane"])), ("random", random_rays(torch, np))):
        n = o.shape[0]
        kinds = dict(hit=torch.uint8, t=torch.float64, u=torch.float64, v=torch.float64, tri=torch.int32)
        five = {k: torch.empty(n, dtype=dt, device="cuda") for k, dt in kinds.items()}
        occ = torch.empty(n, dtype=torch.uint8, device="cuda")
        ho, hd, hm = o.cpu().numpy(), d.cpu().numpy(), None if m is None else m.cpu().numpy()
        rows = {}
        for mode, rt in rts.items():
            launch = dict(occluded=lambda: rt.occluded_into(o, d, occ, m), intersect_all=lambda: rt.intersect_rays_into(o, d, five, m),
                          intersect_hit_only=lambda: rt.intersect_rays_into(o, d, {"hit": five["hit"]}, m))
            ms = {k: [] for k in KINDS}
            wall_dev = []
            for i in range(WARMUP + launches):                                  # alternating: one launch of each kind per round
                for k in KINDS:
                    t0 = time.perf_counter(); launch[k](); torch.cuda.synchronize(); dt = (time.perf_counter() - t0) * 1e3
                    if i >= WARMUP:
                        ms[k].append(rt.last_stats()["kernel_ms"])
                        if k == "intersect_all": wall_dev.append(dt)
            rt.occluded_into(o, d, occ, m); rt.intersect_rays_into(o, d, five, m); torch.cuda.synchronize()
            assert bool((occ == five["hit"]).all()), (scene, name, mode)        # faster and different is not faster
            wall_host = []
            for _ in range(HOST_REPS):
                t0 = time.perf_counter(); got = rt.intersect_rays(ho, hd, hm); wall_host.append((time.perf_counter() - t0) * 1e3)
            assert np.array_equal(got[0], occ.cpu().numpy().astype(bool)), (scene, name, mode)
            med = {k: statistics.median(v) for k, v in ms.items()}
            row = {f"{k}_kernel_ms": round(med[k], 4) for k in KINDS}
            row.update({f"{k}_kernel_ms_min_max": [round(min(ms[k]), 4), round(max(ms[k]), 4)] for k in KINDS})
            row["intersect_all_relative_spread"] = round((max(ms["intersect_all"]) - min(ms["intersect_all"])) / med["intersect_all"], 4)
            row["occluded_over_intersect_all"] = round(med["occluded"] / med["intersect_all"], 3)
            row["intersect_hit_only_over_intersect_all"] = round(med["intersect_hit_only"] / med["intersect_all"], 3)
            row["host_form_intersect_rays_wall_ms"] = round(statistics.median(wall_host), 2)
            row["intersect_rays_into_plus_synchronize_wall_ms"] = round(statistics.median(wall_dev), 4)
            rows[mode] = row
        out["ray_sets"][name] = dict(rays=n, occluded_fraction=round(float(occ.float().mean()), 4), walks=rows)
        del five, occ, o, d, m
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20); ap.add_argument("--scenes", default="teapot,soup100000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ray_batches.json")); ap.add_argument("--child", default=None)
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
