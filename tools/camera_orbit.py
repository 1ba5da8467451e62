"""Developer tool: what a moving camera costs (rrt_raytracer_set_camera).  N poses on a circle around a target, every pose looking at it:
  * HIP-event ms per frame over the orbit (min / median / max), per forced walk variant and for the default, beside the default pose's frame of the same build;
  * wall time of set_camera with a changed eye (median over the orbit: the exactness guard is searched again on the GPU) and with an unchanged eye (a
    pure rotation: no GPU work), beside the create_ms of the raytracer it spares the host from re-creating.
Scenes: the teapot at 1920 x 1080 and the 1 M-triangle soup at 3840 x 2160.  One JSON: profiles/camera_orbit.json.
   python tools/camera_orbit.py [--poses 12] [--scenes teapot,soup1m] [--out profiles/camera_orbit.json]
Every scene is measured in a child process of its own under a time limit; the first failure stops the run."""
import argparse, importlib, json, math, os, statistics, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = {"teapot": dict(size=(1920, 1080), target=(0.0, 1.0, 0.0), limit_s=240), "soup1m": dict(size=(3840, 2160), target=(0.0, 3.0, 0.0), limit_s=420)}
RADIUS, EYE_Y = 10.0, 2.0                       # the reference's camera (0, 2, -10) is pose 0 of the circle


def orbit(n):
    return [(RADIUS * math.sin(2 * math.pi * k / n), EYE_Y, -RADIUS * math.cos(2 * math.pi * k / n)) for k in range(n)]


def spread(v):
    return dict(min=round(min(v), 4), median=round(statistics.median(v), 4), max=round(max(v), 4))


def measure(scene, n_poses):
    import torch
    sys.path.insert(0, ROOT)
    rrt = importlib.import_module("rust-ray-tracer_amd"); syn = importlib.import_module("rust-ray-tracer_amd.synthetic")
    A = os.path.join(ROOT, "assets")
    path = os.path.join(A, "model2.obj") if scene == "teapot" else syn.ensure_soup(A, 1000000, syn.SEED_1M)
    (w, h), target = SCENES[scene]["size"], SCENES[scene]["target"]
    sd = rrt.parse_obj_file(path)
    fb = torch.empty((h, w), dtype=torch.int32, device="cuda")
    poses = orbit(n_poses)

    def frame_ms(rt, frames=3):                 # the last of a few frames: the first of a pose warms caches (and, for the default, the second of a size tunes)
        for _ in range(frames):
            rt.render_into(fb, w, h); torch.cuda.synchronize()
        return rt.last_stats()["kernel_ms"]

    out = dict(scene=scene, size=f"{w}x{h}", poses=n_poses, target=target, radius=RADIUS, eye_y=EYE_Y, walks={})
    for mode in ("lane", "bundle", "ray", None):
        rt = rrt.RayTracer(sd, rrt.default_lights(), box_filter=mode)
        default_ms = frame_ms(rt, 4)
        ms, moved = [], []
        for eye in poses:
            cam = rrt.look_at(eye, target)
            t0 = time.perf_counter(); rt.set_camera(**cam); moved.append((time.perf_counter() - t0) * 1e3)
            ms.append(frame_ms(rt))
        row = dict(default_pose_ms=round(default_ms, 4), orbit_ms=spread(ms), orbit_median_over_default_pose=round(statistics.median(ms) / default_ms, 3))
        if mode is None:
            row["variant_kept"] = rrt.VARIANT_NAMES[rt.last_stats()["filter_variant"]]
            still = []
            for k in range(200):                # unchanged eye, another basis each time
                cam = rrt.look_at(poses[-1], (target[0] + 0.01 * k, target[1], target[2]))
                t0 = time.perf_counter(); rt.set_camera(**cam); still.append((time.perf_counter() - t0) * 1e3)
            out["set_camera_changed_eye_ms"] = spread(moved)
            out["set_camera_unchanged_eye_ms"] = spread(still)
            out["create_ms"] = round(rt.setup_times()["create_ms"], 3)
            out["origin_plane_triangles_last_pose"] = rt.last_stats()["origin_plane_triangles"]
        out["walks"][mode or "default"] = row
        del rt
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=12); ap.add_argument("--scenes", default="teapot,soup1m")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "camera_orbit.json")); ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(measure(a.child, a.poses)), flush=True)
        return 0
    results = []
    for scene in a.scenes.split(","):
        if scene not in SCENES:
            print(f"unknown scene {scene}", file=sys.stderr); return 2
        try:                                    # a fresh process per scene, under its own time limit; nothing more is started after a failure
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", scene, "--poses", str(a.poses)], capture_output=True, text=True, timeout=SCENES[scene]["limit_s"])
        except subprocess.TimeoutExpired:
            print(f"{scene}: no result within {SCENES[scene]['limit_s']} s; stopping", file=sys.stderr); return 124
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(f"{scene}: exit status {r.returncode}; stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr); return r.returncode or 1
        results.append(json.loads(line[0][7:])); print(json.dumps(results[-1]), flush=True)
    json.dump(results, open(a.out, "w"), indent=1)
    print(f"wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
