"""Developer tool: what the on-device compaction of ray batches and records costs and buys (rrt_compact_rays_device, rrt_scatter_rays_device).
Per scene, on record sets that are built on the device once and are the same for every timing, the GPU time between two events on the stream as the median of
--launches runs after warm-up with the spread (min, max):
  (a) the compaction launch -- HIT over `material`; point, normal, material and rot gathered, index and count written -- beside what a caller had before on the
      same tensors: torch nonzero (which synchronises the host) + one index_select per array.  The survivors of both are compared byte for byte; bytes moved per
      second = (the bytes read of the selection and of the survivors + the bytes written of all n slots) / time;
  (b) per forced walk, n = 8 and 16 directions at max_t 2.0, with and without a rotation per record: compaction + rrt_ambient_rays_device on the n PADDED records +
      two scatters (occluded, open) beside rrt_ambient_rays_device on the raw records, and beside the kernel of rrt_occluded_rays_device on the same rays as
      profiles/ambient_rays.json recorded it (read from that file when it holds the case).  The scattered masks are compared with the raw call's, bit for bit;
  (c) the level-1 rays of a frame as a batch of fixed size -- next_origin / next_dir of every traced sub-sample, a level-0 miss being a dead ray --: compaction
      (HIT over the level-0 `material`, the rays gathered, max_t synthesised) + rrt_surface_rays_device with `lights` on the n padded rays beside the same call on
      the raw batch with max_t = NaN for the dead rays.  point, normal, material and lights of the survivors are compared byte for byte.
  The expectation that is recorded, not enforced: on record sets with about half misses the compacted pipeline takes no longer than the raw call.
Record sets:  "level1" = the level-1 records of every hit sub-sample of the 1920 x 1080 frame;  "frame_planes" = the frame's own planes, flattened (the sets of
tools/ambient_rays_bench.py).  Scenes: the teapot and the 100 k-triangle soup.  One JSON: profiles/compact.json.
   python tools/compact_bench.py [--launches 20] [--scenes teapot,soup100k] [--walks lane,bundle,ray] [--out profiles/compact.json]
Every scene is measured in a child process of its own under `timeout -k 10`; the first failure stops the run."""
import argparse, importlib, json, math, os, statistics, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ambient_bench import table
from ray_surface_bench import H, W, device_arrays

SCENES = {"teapot": 400, "soup100k": 900}       # time limit of the child, seconds
WARMUP = 2
MAX_T = 2.0
SETTINGS = tuple((n, rot) for n in (8, 16) for rot in (False, True))
INPUTS = ("point", "normal", "material")
GOLDEN = 0.6180339887498949
ELEM = dict(point=24, normal=24, material=4, rot=16, origins=24, dirs=24, max_t=8)


def primary_rays(torch, rt):
    """origins and directions of every traced sub-sample of the W x H frame in the creation pose, formed on the device (rrt.h: rrt_camera)"""
    cam = rt.camera()
    f64 = dict(dtype=torch.float64, device="cuda")
    x = torch.arange(W, **f64) - (W // 2); y = (H - H // 2) - torch.arange(1, H, **f64)       # (canvas row 0 is never traced)
    a = torch.stack([x, x + 0.5, x, x + 0.5], -1) * (1.0 / W)
    b = torch.stack([y, y, y + 0.5, y + 0.5], -1) * (1.0 / H)
    R, U, F = (torch.tensor(cam[k], **f64) for k in ("right", "up", "forward"))
    d = ((R * a[None, :, :, None] + U * b[:, None, :, None]) + F * 1.0).reshape(-1, 3).contiguous()
    return torch.tensor(cam["eye"], **f64).expand_as(d).contiguous().view(-1), d.view(-1)


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
    try:
        recorded = {r["scene"]: r for r in json.load(open(os.path.join(ROOT, "profiles", "ambient_rays.json")))}.get(scene, {}).get("record_sets", {})
    except (OSError, ValueError):
        recorded = {}

    def timed(launch):
        ms = []
        for i in range(WARMUP + launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); launch(); e1.record(); torch.cuda.synchronize()
            if i >= WARMUP: ms.append(e0.elapsed_time(e1))
        return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4))

    # ---- level 0 of the frame, and the record sets, built once
    o0, d0 = primary_rays(torch, first)
    n0 = o0.numel() // 3
    l0 = device_arrays(torch, rrt, n0, ("material", "next_origin", "next_dir"))
    first.surface_rays_into(o0, d0, l0); torch.cuda.synchronize()
    del o0, d0
    seen = (l0["material"] >= 0) & (l0["material"] < n_mats)
    sets = {}
    ro, rd = l0["next_origin"].view(-1, 3)[seen].contiguous().view(-1), l0["next_dir"].view(-1, 3)[seen].contiguous().view(-1)
    rec = device_arrays(torch, rrt, ro.numel() // 3, INPUTS)
    first.surface_rays_into(ro, rd, rec); torch.cuda.synchronize()
    sets["level1"] = rec
    del ro, rd
    planes = dict(point=torch.empty((H, W, 4, 3), **f64), normal=torch.empty((H, W, 4, 3), **f64), material=torch.empty((H, W, 4), **i32))
    first.surface_into(planes, W, H); torch.cuda.synchronize()
    sets["frame_planes"] = {k: v.view(-1) for k, v in planes.items()}

    out = dict(scene=scene, size=f"{W}x{H}", launches=launches, triangles=sd.info["n_tris"], max_t=MAX_T, record_sets={})
    for set_name, rec in sets.items():
        n = rec["material"].numel()
        i = torch.arange(n, **f64) * GOLDEN
        a = 2.0 * math.pi * (i - torch.floor(i))
        src = dict(rec, rot=torch.stack([torch.cos(a), torch.sin(a)], -1).contiguous().view(-1))
        del i, a
        packed = {k: torch.empty_like(t) for k, t in src.items()}
        index, count = torch.empty(n, **i32), torch.empty(1, **i32)
        scratch = torch.empty(first.compact_scratch_bytes(n), dtype=torch.uint8, device="cuda")
        # (a)
        res = dict(records=n, scratch_bytes=scratch.numel())
        res["compact"] = timed(lambda: first.compact_rays_into(packed, src, "hit", index, count, scratch))
        hits = int(count.cpu().numpy().view("uint32")[0])
        res["hits"], res["hit_fraction"] = hits, round(hits / n, 4)
        moved = n * 4 + hits * sum(ELEM[k] for k in src) + n * (4 + sum(ELEM[k] for k in src))
        res["compact_bytes"] = moved
        res["compact_gbytes_per_s"] = round(moved / res["compact"]["median_ms"] / 1e6, 1)
        by_torch = {}

        def torch_path():
            idx = ((src["material"] >= 0) & (src["material"] < n_mats)).nonzero().squeeze(1)
            by_torch.update(index=idx, **{k: t.view(n, -1).index_select(0, idx) for k, t in src.items()})
        res["torch_nonzero_index_select"] = timed(torch_path)
        if by_torch["index"].numel() != hits or not torch.equal(by_torch["index"].to(torch.int32), index[:hits]):
            raise SystemExit(f"{scene}, {set_name}: index differs from torch nonzero")
        for k in src:
            if not torch.equal(by_torch[k].contiguous().view(-1).view(torch.uint8), packed[k].view(n, -1)[:hits].contiguous().view(-1).view(torch.uint8)):
                raise SystemExit(f"{scene}, {set_name}: the gathered {k} differs from torch index_select")
        if int((index[hits:] != -1).sum()) or int((packed["material"][hits:] != -1).sum()):
            raise SystemExit(f"{scene}, {set_name}: the tail is not dead")
        res["compact_over_torch"] = round(res["compact"]["median_ms"] / res["torch_nonzero_index_select"]["median_ms"], 3)
        by_torch.clear()
        print(f"{scene}, {set_name}, (a): {json.dumps(res)}", file=sys.stderr, flush=True)
        # (b)
        raw_out = dict(occluded=torch.empty(n, **i32), open=torch.empty(n, **i32))
        pad_out = dict(occluded=torch.empty(n, **i32), open=torch.empty(n, **i32))
        final = dict(occluded=torch.empty(n, **i32), open=torch.empty(n, **i32))
        rows = {}
        for mode, rt in rts.items():
            row = {}
            for ns, with_rot in SETTINGS:
                dirs = table(ns)
                names = INPUTS + (("rot",) if with_rot else ())

                def pipeline():
                    rt.compact_rays_into({k: packed[k] for k in names}, {k: src[k] for k in names}, "hit", index, count, scratch)
                    rt.ambient_rays_into(pad_out, {k: packed[k] for k in INPUTS}, dirs, MAX_T, rot_t=packed["rot"] if with_rot else None)
                    rt.scatter_rays_into(index, pad_out["occluded"], final["occluded"])
                    rt.scatter_rays_into(index, pad_out["open"], final["open"])
                r = dict(raw=timed(lambda: rt.ambient_rays_into(raw_out, rec, dirs, MAX_T, rot_t=src["rot"] if with_rot else None)))
                final["occluded"].zero_(); final["open"].fill_(ns)
                r["compacted"] = timed(pipeline)
                what = f"{scene}, {set_name}, walk {mode}, n {ns}, rot {with_rot}"
                if not torch.equal(final["occluded"], raw_out["occluded"]) or not torch.equal(final["open"], raw_out["open"]):
                    raise SystemExit(f"{what}: the scattered results of the padded batch differ from the raw call's")
                r["compacted_over_raw"] = round(r["compacted"]["median_ms"] / r["raw"]["median_ms"], 3)
                r["compacted_no_longer_than_raw"] = bool(r["compacted"]["median_ms"] <= r["raw"]["median_ms"])
                key = f"n{ns}_max_t_{MAX_T}_{'rot' if with_rot else 'no_rot'}"
                batch = recorded.get(set_name, {}).get("walks", {}).get(mode, {}).get(key, {}).get("occluded_rays_device")
                if batch:
                    r["recorded_occluded_rays_device_ms"] = batch["median_ms"]
                    r["compacted_over_recorded_occluded_rays_device"] = round(r["compacted"]["median_ms"] / batch["median_ms"], 3)
                row[key] = r
                print(f"{what}: {json.dumps(r)}", file=sys.stderr, flush=True)
            rows[mode] = row
        res["ambient"] = rows
        out["record_sets"][set_name] = res
        del src, packed, index, count, raw_out, pad_out, final
    # (c)
    n = n0
    src = dict(material=l0["material"], origins=l0["next_origin"], dirs=l0["next_dir"])
    rays = dict(origins=torch.empty(3 * n, **f64), dirs=torch.empty(3 * n, **f64), max_t=torch.empty(n, **f64))
    index, count = torch.empty(n, **i32), torch.empty(1, **i32)
    scratch = torch.empty(first.compact_scratch_bytes(n), dtype=torch.uint8, device="cuda")
    dead = torch.where(seen, torch.full((n,), math.inf, **f64), torch.full((n,), math.nan, **f64))
    names = INPUTS + ("lights",)
    raw_out, pad_out = device_arrays(torch, rrt, n, names), device_arrays(torch, rrt, n, names)
    hits = int(seen.sum())
    res = dict(rays=n, alive=hits, alive_fraction=round(hits / n, 4), walks={})
    for mode, rt in rts.items():
        def pipeline():
            rt.compact_rays_into(rays, src, "hit", index, count, scratch)
            rt.surface_rays_into(rays["origins"], rays["dirs"], pad_out, max_t_t=rays["max_t"])
        r = dict(raw=timed(lambda: rt.surface_rays_into(src["origins"], src["dirs"], raw_out, max_t_t=dead)), compacted=timed(pipeline))
        idx = index[:hits].long()
        for k in names:
            w = 3 if k in ("point", "normal") else 1
            if not torch.equal(raw_out[k].view(n, w).index_select(0, idx).contiguous().view(-1).view(torch.uint8), pad_out[k].view(n, w)[:hits].contiguous().view(-1).view(torch.uint8)):
                raise SystemExit(f"{scene}, surface rays, walk {mode}: {k} of the padded batch differs from the raw call's")
        r["compacted_over_raw"] = round(r["compacted"]["median_ms"] / r["raw"]["median_ms"], 3)
        r["compacted_no_longer_than_raw"] = bool(r["compacted"]["median_ms"] <= r["raw"]["median_ms"])
        res["walks"][mode] = r
        print(f"{scene}, surface rays with lights, walk {mode}: {json.dumps(r)}", file=sys.stderr, flush=True)
    out["surface_rays_level1"] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20); ap.add_argument("--scenes", default="teapot,soup100k"); ap.add_argument("--walks", default="lane,bundle,ray")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compact.json")); ap.add_argument("--child", default=None)
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
