"""Developer tool: what a frame traced as compacted ray generations costs beside the fused frame kernel, and what the two ends of the per-ray pipeline cost
(rrt_render_wavefront_device, rrt_frame_rays_device, rrt_mix_rays_device, rrt_mix_pixels_device).  Per scene at 1920 x 1080, the GPU time between two events on
the stream as the median of --launches runs after warm-up with the spread (min, max):
  (a) per forced walk and per entry order: rrt_render_wavefront_device beside rrt_render_device; every timed frame is compared with rrt_render_device's;
  (b) per forced walk and per entry order: the stages of (a) from library calls, each timed on its own -- the frame rays, and per level the surface records,
      local / kr, the compaction of the mirror hits; back up the scatter and the mix of a level; the pixels -- with the rays alive per level;
  (c) rrt_frame_rays_device with all three arrays, per order, in bytes written per second, beside torch forming the same directions on the device
      (tools/compact_bench.py: primary_rays) -- profiles/compact.json has the rate the compaction launch reaches on arrays of the same kind;
  (d) rrt_mix_rays_device on level 0 of the frame and rrt_mix_pixels_device beside their restatements in torch (tests/test_gpu_shade_rays.py: the unwind of
      test_the_recursion_from_library_calls_alone; Color::mix as channel sums).
Nothing here is a gate: whatever comes out is recorded, cases that lose included.
Scenes: the teapot and the 100 k-triangle soup.  One JSON: profiles/wavefront.json.
   python tools/wavefront_bench.py [--launches 20] [--scenes teapot,soup100k] [--walks lane,bundle,ray] [--out profiles/wavefront.json]
Every scene is measured in a child process of its own under `timeout -k 10`; the first failure stops the run."""
import argparse, importlib, json, os, statistics, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from compact_bench import H, W, primary_rays

SCENES = {"teapot": 400, "soup100k": 700}       # time limit of the child, seconds
WARMUP = 2
ORDER_NAMES = ("rows", "tiles")


def measure(scene, launches, walks):
    import torch
    sys.path.insert(0, ROOT)
    rrt = importlib.import_module("rust-ray-tracer_amd"); syn = importlib.import_module("rust-ray-tracer_amd.synthetic")
    A = os.path.join(ROOT, "assets")
    sd = rrt.parse_obj_file(os.path.join(A, "model2.obj") if scene == "teapot" else syn.ensure_soup(A, 100000, syn.SEED_100K))
    n_mats = sd.info["n_mats"]
    f64, i32 = dict(dtype=torch.float64, device="cuda"), dict(dtype=torch.int32, device="cuda")
    rts = {mode: rrt.RayTracer(sd, rrt.default_lights(), box_filter=mode) for mode in walks}
    first = next(iter(rts.values()))
    depth_max = rrt.MAX_REFLECTION_DEPTH

    def timed(launch):
        ms = []
        for i in range(WARMUP + launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); launch(); e1.record(); torch.cuda.synchronize()
            if i >= WARMUP: ms.append(e0.elapsed_time(e1))
        return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4))

    out = dict(scene=scene, launches=launches, triangles=sd.info["n_tris"], width=W, height=H, max_reflection_depth=depth_max, walks={})
    want = torch.empty(W * H, **i32)
    fb = torch.empty(W * H, **i32)
    for mode, rt in rts.items():
        row = dict(render=timed(lambda: rt.render_into(want, W, H)), orders={})
        for order, oname in enumerate(ORDER_NAMES):
            n = rrt.frame_ray_count(W, H, None, order)
            need = rt.wavefront_work_bytes(W, H, None, order)
            work = torch.empty(need, dtype=torch.uint8, device="cuda")

            def frame():
                rt.render_wavefront_into(fb, work, W, H, order=order)
                if not torch.equal(fb, want):
                    raise SystemExit(f"{scene}, walk {mode}, order {oname}: the frame by generations differs from rrt_render_device's")
            # (a): the comparison sits outside the two events of the timing below
            frame()
            r = dict(entries=n, work_bytes=need, wavefront=timed(lambda: rt.render_wavefront_into(fb, work, W, H, order=order)))
            frame()
            r["wavefront_over_render"] = round(r["wavefront"]["median_ms"] / row["render"]["median_ms"], 3)
            del work
            # (b): the same stages from library calls, each on its own
            F8 = lambda k: torch.empty(k * n, **f64)
            I4 = lambda k=n: torch.empty(k, **i32)
            rays = [dict(origins=F8(3), dirs=F8(3), max_t=F8(1)) for _ in range(2)]
            rec = dict(albedo=I4(), point=F8(3), normal=F8(3), lights=I4(), next_origin=F8(3), next_dir=F8(3))
            kept = [dict(local=F8(3), kr=F8(1), material=I4(), index=I4(), count=I4(1)) for _ in range(depth_max + 1)]
            colour, reflected = [I4(), I4()], I4()
            scratch = torch.empty(max(1, rt.compact_scratch_bytes(n)), dtype=torch.uint8, device="cuda")
            stages = dict(frame_rays=timed(lambda: rt.frame_rays_into(rays[0], W, H, order=order)), levels=[])
            for k in range(depth_max + 1):
                cur, nxt, K = rays[k & 1], rays[(k & 1) ^ 1], kept[k]
                records = dict(rec, material=K["material"])
                if k == depth_max:
                    records = {name: t for name, t in records.items() if not name.startswith("next_")}
                lv = dict(surface=timed(lambda: rt.surface_rays_into(cur["origins"], cur["dirs"], records, max_t_t=cur["max_t"])),
                          shade=timed(lambda: rt.shade_rays_into(dict(local=K["local"], kr=K["kr"]), cur["dirs"], records, depth=k)))
                if k < depth_max:
                    src = dict(origins=rec["next_origin"], dirs=rec["next_dir"], material=K["material"])
                    lv["compact"] = timed(lambda: rt.compact_rays_into(nxt, src, "mirror", K["index"], K["count"], scratch))
                    lv["alive_below"] = int(K["count"].cpu().numpy().view("uint32")[0])
                stages["levels"].append(lv)
            for k in reversed(range(depth_max + 1)):
                K, lv = kept[k], stages["levels"][k]
                if k < depth_max:
                    lv["scatter"] = timed(lambda: rt.scatter_rays_into(K["index"], colour[(k + 1) & 1], reflected))
                lv["mix"] = timed(lambda: rt.mix_rays_into(colour[k & 1], K["local"], kr_t=K["kr"], reflected_t=reflected if k < depth_max else None, material_t=K["material"]))
            stages["mix_pixels"] = timed(lambda: rt.mix_pixels_into(fb, colour[0], W, H, order=order))
            if not torch.equal(fb, want):
                raise SystemExit(f"{scene}, walk {mode}, order {oname}: the frame from the stages differs from rrt_render_device's")
            stages["sum_ms"] = round(stages["frame_rays"]["median_ms"] + stages["mix_pixels"]["median_ms"]
                                     + sum(v["median_ms"] for lv in stages["levels"] for v in lv.values() if isinstance(v, dict)), 4)
            r["stages"] = stages
            if mode == walks[0]:
                # (c)
                g = dict(frame_rays=stages["frame_rays"], bytes=56 * n)
                g["gbytes_per_s"] = round(g["bytes"] / g["frame_rays"]["median_ms"] / 1e6, 1)
                if order == 0:
                    g["torch_directions"] = timed(lambda: primary_rays(torch, rt))
                r["generator"] = g
                # (d)
                K = kept[0]
                q = lambda x: torch.where(x > 0.0, torch.clamp(x, max=255.0), torch.zeros_like(x)).to(torch.int64)
                packed = lambda c: (c[:, 0] << 16) | (c[:, 1] << 8) | c[:, 2]

                def torch_mix():
                    local, kr, below = K["local"].view(-1, 3), K["kr"], reflected.long()
                    ch = torch.stack([(below >> 16) & 255, (below >> 8) & 255, below & 255], -1).to(torch.float64)
                    c = torch.where((kr > 0.0)[:, None], local * (1.0 - kr)[:, None] + ch * kr[:, None], local)      # raytracer.rs:89-101
                    return torch.where((K["material"].long() & 0xFFFFFFFF) < n_mats, packed(q(c)), torch.full_like(below, 0xFFFFFF))

                def torch_pixels():
                    c = colour[0].long().view(-1, 4)
                    return ((((c >> 16) & 255).sum(1) >> 2) << 16) | ((((c >> 8) & 255).sum(1) >> 2) << 8) | ((c & 255).sum(1) >> 2)
                if not torch.equal(torch_mix().to(torch.int32), colour[0]):
                    raise SystemExit(f"{scene}, order {oname}: rrt_mix_rays_device differs from the torch restatement on level 0")
                r["mix_rays"] = dict(library=stages["levels"][0]["mix"], torch=timed(torch_mix))
                r["mix_pixels"] = dict(library=stages["mix_pixels"], torch_rows_order_sums=timed(torch_pixels))
            del rays, rec, kept, colour, reflected, scratch
            row["orders"][oname] = r
            print(f"{scene}, walk {mode}, order {oname}: {json.dumps(r)}", file=sys.stderr, flush=True)
        out["walks"][mode] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20); ap.add_argument("--scenes", default="teapot,soup100k"); ap.add_argument("--walks", default="lane,bundle,ray")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wavefront.json")); ap.add_argument("--child", default=None)
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
        # a fresh process per scene under its own time limit; nothing more is started after a failure
        r = subprocess.run(["timeout", "-k", "10", str(SCENES[scene]), sys.executable, os.path.abspath(__file__), "--child", scene, "--launches", str(a.launches),
                            "--walks", a.walks], stdout=subprocess.PIPE, text=True)
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(f"{scene}: exit status {r.returncode}; stopping\n{r.stdout[-2000:]}", file=sys.stderr); return r.returncode or 1
        results.append(json.loads(line[0][7:])); print(json.dumps(results[-1]), flush=True)
    json.dump(results, open(a.out, "w"), indent=1)
    print(f"wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
