"""Developer tool: what ambient occlusion from kept surface buffers costs (rrt_ambient_surface_device) beside the same rays as a device-resident batch
(rrt_occluded_rays_device).  Per scene, per forced walk variant and per sample table (n = 8 and 16 directions, max_t = 2.0 and +inf), HIP-event kernel_ms as the
median of --launches launches after warm-up, with the spread (min, max):
  (1) the fused launch writing `occluded` only;
  (2) the fused launch writing `occluded` and `grey`;
  (3) the yardstick: rrt_occluded_rays_device with the same walk forced on the very same rays -- those of every hit of the WHOLE frame, formed by torch on the
      device from the kept planes in the contract's operation order (origins 24 B, directions 24 B and max_t 8 B per ray in device memory), ray k of hit j at
      index k * hits + j, hits in plane order.  The forming is timed separately (torch events, median of 3): it is what a host without the fused launch pays on
      top of the walk.
The masks of (1) are compared with the bytes of (3), bit for bit; a difference fails the run.
Scenes: the teapot and the 100 k-triangle soup, both at 1920 x 1080 in the creation pose.  One JSON: profiles/ambient.json.
   python tools/ambient_bench.py [--launches 20] [--scenes teapot,soup100k] [--walks lane,bundle,ray] [--out profiles/ambient.json]
Every scene is measured in a child process of its own under a time limit; the first failure stops the run."""
import argparse, importlib, json, math, os, statistics, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 1920, 1080
SCENES = {"teapot": 420, "soup100k": 900}       # time limit of the child, seconds
WARMUP = 2
TABLES = ((8, 2.0), (16, 2.0), (8, math.inf), (16, math.inf))


def table(n):
    """n directions in the tangent frame: phi = 2 pi (k + 0.5) / n, cos(theta) = (0.3, 0.6, 0.85, 0.45)[k % 4] (n = 8: the table of tests/ambient_checks.py)."""
    out = []
    for k in range(n):
        phi, c = 2.0 * math.pi * (k + 0.5) / n, (0.3, 0.6, 0.85, 0.45)[k % 4]
        s = math.sqrt(1.0 - c * c)
        out.append((s * math.cos(phi), s * math.sin(phi), c))
    return out


def measure(scene, launches, walks):
    import torch
    sys.path.insert(0, ROOT)
    rrt = importlib.import_module("rust-ray-tracer_amd"); syn = importlib.import_module("rust-ray-tracer_amd.synthetic")
    A = os.path.join(ROOT, "assets")
    sd = rrt.parse_obj_file(os.path.join(A, "model2.obj") if scene == "teapot" else syn.ensure_soup(A, 100000, syn.SEED_100K))
    n_mats = sd.info["n_mats"]
    f64 = dict(dtype=torch.float64, device="cuda")
    planes = dict(point=torch.empty((H, W, 4, 3), **f64), normal=torch.empty((H, W, 4, 3), **f64), material=torch.empty((H, W, 4), dtype=torch.int32, device="cuda"))
    occluded = torch.empty((H, W, 4), dtype=torch.int32, device="cuda")
    grey = torch.empty((H, W), dtype=torch.int32, device="cuda")

    def timed(rt, launch):
        ms = []
        for i in range(WARMUP + launches):
            launch(); torch.cuda.synchronize()
            if i >= WARMUP: ms.append(rt.last_stats()["kernel_ms"])
        return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4))

    # engine.rs:85-99 on [m][3] tensors: one torch kernel per operation, each rounded on its own
    def cross(a, b):
        return torch.stack([a[:, 1] * b[2] - a[:, 2] * b[1], -(a[:, 0] * b[2] - a[:, 2] * b[0]), a[:, 0] * b[1] - a[:, 1] * b[0]], 1)

    def cross2(a, b):
        return torch.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], -(a[:, 0] * b[:, 2] - a[:, 2] * b[:, 0]), a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)

    def length(a):
        return torch.sqrt(a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1] + a[:, 2] * a[:, 2])

    def form(idx, dirs, max_t):
        """origins, directions and max_t of the rays of the hits idx (indices of sub-samples), ray k of hit j at k * len(idx) + j"""
        p, n = planes["point"].view(-1, 3)[idx], planes["normal"].view(-1, 3)[idx]
        tg = cross(n, (0.0, 1.0, 0.0))
        zero = length(tg) == 0.0
        tg = torch.where(zero[:, None], cross(n, (0.0, 0.0, 1.0)), tg)
        tg = tg / length(tg)[:, None]
        bt = cross2(n, tg)
        bt = bt / length(bt)[:, None]
        o = p + n * 1e-4                                     # surface_offset of the default options
        D = torch.cat([(tg * sx + bt * sy) + n * sz for sx, sy, sz in dirs])
        O = o.repeat(len(dirs), 1)
        return O, D, torch.full((len(D),), max_t, **f64)

    out = dict(scene=scene, size=f"{W}x{H}", launches=launches, triangles=sd.info["n_tris"], yardstick_region="the whole frame", walks={})
    for mode in walks:
        rt = rrt.RayTracer(sd, rrt.default_lights(), box_filter=mode)
        rt.surface_into(planes, W, H); torch.cuda.synchronize()
        mat = planes["material"].view(-1)
        idx = ((mat >= 0) & (mat < n_mats)).nonzero().squeeze(1)
        hits = int(idx.numel())
        row = dict(hits=hits, rays_hit_fraction=round(hits / mat.numel(), 4), tables={})
        for n, max_t in TABLES:
            dirs = table(n)
            r = dict(rays=hits * n)
            r["fused_occluded"] = timed(rt, lambda: rt.ambient_into(dict(occluded=occluded), planes, dirs, max_t, W, H))
            r["fused_occluded_and_grey"] = timed(rt, lambda: rt.ambient_into(dict(occluded=occluded, grey=grey), planes, dirs, max_t, W, H))
            form_ms = []
            for _ in range(3):
                O = D = M = None
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); O, D, M = form(idx, dirs, max_t); e1.record(); torch.cuda.synchronize()
                form_ms.append(e0.elapsed_time(e1))
            r["forming_ms"] = dict(median_ms=round(statistics.median(form_ms), 3), min_ms=round(min(form_ms), 3), max_ms=round(max(form_ms), 3))
            r["ray_bytes"] = int(O.numel() * 8 + D.numel() * 8 + M.numel() * 8)
            byte = torch.empty((len(D),), dtype=torch.uint8, device="cuda")
            r["yardstick_occluded_rays_device"] = timed(rt, lambda: rt.occluded_into(O.view(-1), D.view(-1), byte, M))
            masks = occluded.view(-1)[idx]
            bits = ((masks[None, :] >> torch.arange(n, dtype=torch.int32, device="cuda")[:, None]) & 1).to(torch.uint8)
            if not torch.equal(bits, byte.view(n, hits)):
                raise SystemExit(f"{scene}, walk {mode}, n {n}, max_t {max_t}: {int((bits != byte.view(n, hits)).sum())} bits of the fused masks differ from rrt_occluded_rays_device")
            if int(((masks >> n) != 0).sum()) or int((occluded.view(-1) != 0).sum()) != int((masks != 0).sum()):
                raise SystemExit(f"{scene}, walk {mode}, n {n}: bits at or above n, or bits of a miss, are set")
            r["occluded_fraction"] = round(float(byte.sum(dtype=torch.int64)) / len(D), 4)
            r["fused_occluded_over_yardstick"] = round(r["fused_occluded"]["median_ms"] / r["yardstick_occluded_rays_device"]["median_ms"], 3)
            r["fused_both_over_yardstick"] = round(r["fused_occluded_and_grey"]["median_ms"] / r["yardstick_occluded_rays_device"]["median_ms"], 3)
            row["tables"][f"n{n}_max_t_{'inf' if math.isinf(max_t) else max_t}"] = r
            print(f"{scene}, walk {mode}, n {n}, max_t {max_t}: {json.dumps(r)}", file=sys.stderr, flush=True)   # (progress; the result line goes to stdout)
            del O, D, M, byte, masks, bits
        out["walks"][mode] = row
        del rt
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20); ap.add_argument("--scenes", default="teapot,soup100k"); ap.add_argument("--walks", default="lane,bundle,ray")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ambient.json")); ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.launches < 20:
        print("at least 20 launches", file=sys.stderr); return 2
    walks = a.walks.split(",")
    if not set(walks) <= {"lane", "bundle", "ray"}:
        print(f"unknown walk in {a.walks}", file=sys.stderr); return 2
    if a.child:
        print("RESULT " + json.dumps(measure(a.child, a.launches, walks)), flush=True)
        return 0
    results = []
    for scene in a.scenes.split(","):
        if scene not in SCENES:
            print(f"unknown scene {scene}", file=sys.stderr); return 2
        try:                                    # a fresh process per scene, under its own time limit; nothing more is started after a failure
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", scene, "--launches", str(a.launches), "--walks", a.walks], stdout=subprocess.PIPE, text=True,
                               timeout=SCENES[scene])
        except subprocess.TimeoutExpired:
            print(f"{scene}: no result within {SCENES[scene]} s; stopping", file=sys.stderr); return 124
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(f"{scene}: exit status {r.returncode}; stopping\n{r.stdout[-2000:]}", file=sys.stderr); return r.returncode or 1
        results.append(json.loads(line[0][7:])); print(json.dumps(results[-1]), flush=True)
    json.dump(results, open(a.out, "w"), indent=1)
    print(f"wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
