"""Developer tool: what moving lights and geometry costs on a living raytracer (rrt_raytracer_set_lights, rrt_raytracer_set_triangles,
rrt_raytracer_set_triangles_device) against the only way there was before: rrt_raytracer_destroy + rrt_raytracer_create_from_arrays + rrt_raytracer_set_camera.
Per scene (the teapot; the 1 M-triangle soup with the teapot's materials and textures), in a posed camera at 1920 x 1080, wall time on the host of
  set_lights                                  (mean of 1000 calls);
  set_triangles, set_triangles_device         with the memory an update keeps (the default), and with rrt_raytracer_release_update_memory before every
                                              update (the release is inside the timed span): what keeping the memory is worth;
  destroy + create_from_arrays + set_camera   the same change of geometry without this feature;
and, after each of these, of the first frame (render_into + synchronize): median, minimum and maximum of --reps repetitions (at least 20).  The geometry
alternates between rotations of the scene about y, computed once, on the host and on the device, before anything is timed.
   python tools/scene_update_bench.py [--reps 20] [--scenes teapot,soup1m] [--out profiles/scene_update.json]
Every scene is measured in a child process of its own under `timeout -k 10`; the first failure stops the run."""
import argparse, importlib, json, os, statistics, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 1920, 1080
SCENES = {"teapot": 300, "soup1m": 600}          # time limit of the child, seconds
POSES = 4


def spread(v):
    return dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4))


def measure(scene, reps):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    rrt = importlib.import_module("rust-ray-tracer_amd"); syn = importlib.import_module("rust-ray-tracer_amd.synthetic")
    sd = rrt.parse_obj_file(os.path.join(ROOT, "assets", "model2.obj"))
    mats, texs, lights = sd.materials(), sd.textures(), rrt.default_lights()
    if scene == "teapot":
        pos, uv, nrm, mat = sd.triangles()
    else:
        v, vt, n = syn.soup_arrays(1000000, syn.SEED_1M)
        pos = v; uv = np.concatenate([vt, np.zeros((len(v), 3, 1))], -1); nrm = np.repeat(n[:, None, :], 3, 1); mat = np.zeros(len(v), np.uint32)
    uv = np.ascontiguousarray(uv, np.float64); mat = np.ascontiguousarray(mat, np.uint32)
    host, dev = [], []
    for k in range(POSES):                                                  # the moved geometry, host and device copies, made before anything is timed
        a = 0.05 * (k + 1); c, s = np.cos(a), np.sin(a)
        R = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
        p, q = np.ascontiguousarray(pos @ R.T), np.ascontiguousarray(nrm @ R.T)
        host.append((p, q)); dev.append((torch.from_numpy(p).cuda(), torch.from_numpy(q).cuda()))
    uv_t, mat_t = torch.from_numpy(uv).cuda(), torch.from_numpy(mat.astype(np.int32)).cuda()
    pose = rrt.look_at((3.0, 4.0, -9.0), (0.0, 2.0, 0.0))
    fb = torch.empty(W * H, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def create(k):
        rt = rrt.RayTracer.from_arrays(host[k][0], uv, host[k][1], mat, mats, texs, lights)
        rt.set_camera(**pose)
        return rt

    def frame(rt):
        t0 = time.perf_counter(); rt.render_into(fb, W, H); torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    rt = create(0)
    frame(rt); frame(rt); frame(rt)
    out = dict(scene=scene, triangles=int(len(pos)), reps=reps, frame=[W, H], steady_frame=spread([frame(rt) for _ in range(reps)]))
    other = [rrt.Light.Ambient(0.4), rrt.Light.Point(0.7, rrt.Vector3d(4.0, 6.0, -8.0))]
    t0 = time.perf_counter()
    for i in range(1000):
        rt.set_lights(other if i & 1 else lights)
    out["set_lights_wall_ms"] = round((time.perf_counter() - t0), 6)        # seconds per 1000 calls = ms per call
    rt.set_lights(lights)

    ways = {"set_triangles": lambda k: rt.set_triangles(host[k][0], uv, host[k][1], mat),
            "set_triangles_device": lambda k: rt.set_triangles_from(dev[k][0], uv_t, dev[k][1], mat_t)}
    for name, call in ways.items():
        for keep in (True, False):
            call(1); call(2); frame(rt)                                     # warm-up; the kept memory has reached its size
            wall, first = [], []
            for i in range(reps):
                k = i % POSES
                t0 = time.perf_counter()
                if not keep: rt.release_update_memory()
                call(k)
                wall.append((time.perf_counter() - t0) * 1e3); first.append(frame(rt))
            st = rt.setup_times()
            out[name + ("" if keep else "_memory_released_before_each")] = dict(update_wall=spread(wall), first_frame_after=spread(first),
                                                                                  last_build=dict(octree_ms=round(st["octree_ms"], 3), index_ms=round(st["index_ms"], 3), rest_ms=round(st["upload_ms"], 3)))
    check = rt.render(96, 64)
    rt.release_update_memory()
    wall, first = [], []
    for i in range(reps + 1):                                               # (the first repetition is the warm-up)
        k = i % POSES
        t0 = time.perf_counter()
        rt = None                                                           # rrt_raytracer_destroy
        rt = create(k)
        wall.append((time.perf_counter() - t0) * 1e3); first.append(frame(rt))
    out["destroy_create_from_arrays_set_camera"] = dict(update_wall=spread(wall[1:]), first_frame_after=spread(first[1:]))
    assert np.array_equal(create((reps - 1) % POSES).render(96, 64), check), "the updated raytracer and the re-created one render different frames"
    out["set_triangles_over_recreate"] = round(out["set_triangles"]["update_wall"]["median_ms"] / out["destroy_create_from_arrays_set_camera"]["update_wall"]["median_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20); ap.add_argument("--scenes", default="teapot,soup1m")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_update.json")); ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.reps < 20:
        print("at least 20 repetitions", file=sys.stderr); return 2
    if a.child:
        print("RESULT " + json.dumps(measure(a.child, a.reps)), flush=True)
        return 0
    results = []
    for scene in a.scenes.split(","):
        if scene not in SCENES:
            print(f"unknown scene {scene}", file=sys.stderr); return 2
        # a fresh process per scene under its own time limit; nothing more is started after a failure
        r = subprocess.run(["timeout", "-k", "10", str(SCENES[scene]), sys.executable, os.path.abspath(__file__), "--child", scene, "--reps", str(a.reps)],
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
