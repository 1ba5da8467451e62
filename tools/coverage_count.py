"""Developer tool (CPU only): how many 4x4-pixel waves of a frame the coverage rule proves empty, counted on the host from the triangles of a scene --
and how many more a per-wave test against the projected TRIANGLE would prove for the boxes that cover many waves ("coverage pass";
profiles/coverage_ab.txt).  Also the WIDE boxes of the frame (csrc/coverage_rule.hpp: a box of the root's own list that covers at least WIDE_MIN_WAVES waves and 1 / WIDE_FRAME_SHARE of the frame, at most MAX_WIDE
of them), the SIMPLE waves -- covered, and reached by wide boxes only: render_kernel tests their few triangles instead of walking -- and the wide boxes per simple wave
(profiles/wide_cover_ab.txt).  Creation pose (eye (0, 2, -10), identity basis, viewport 1), boxes padded by 20 / 2^15 as the index pads them below the default root box.
   python tools/coverage_count.py [W H] [scene.obj] [waves above which a box is "huge"]
An approximate restatement in its own arithmetic (the triangles' f64 bounds, not the device's fp32 slot boxes); tests/test_wide_cover_restatement.py holds its wide and
simple counts to tests/wide_cover_checks.py on the teapot at 256 x 144."""
import importlib, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
rrt = importlib.import_module("rust-ray-tracer_amd")
W, H = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (1920, 1080)
scene = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "assets", "model2.obj")
HUGE = int(sys.argv[4]) if len(sys.argv) > 4 else 400
WIDE_MIN_WAVES, WIDE_FRAME_SHARE, MAX_WIDE = 16, 128, 16                # coverage_rule.hpp: kWideMinWaves, kWideFrameShare, kMaxWide
EYE, PAD, MARGIN = np.array([0.0, 2.0, -10.0]), 20.0 / 2 ** 15, 1e-6   # (the pad of a +-20 root box: 2^-15 of the scene magnitude, rrt_stats.filter_pad)
sd = rrt.parse_obj_file(scene)
pos = np.asarray(sd.triangles()[0], np.float64).reshape(-1, 3, 3)
oct_ = sd.octree()
in_root = np.zeros(len(pos), bool); in_root[oct_["own_idx"][oct_["own_off"][0]:oct_["own_off"][1]]] = True   # the root node's own list
keep = (np.abs(pos) <= 20.0).all((1, 2))                            # triangles outside the root box are not in the tree
pos, in_root = pos[keep], in_root[keep]
wx, wy, half_w, top = 2 * ((W + 7) // 8), 2 * ((H + 7) // 8), W // 2, H - H // 2


def project(P):                                                      # [..., 3] -> xd, yd, gamma
    d = P - EYE
    return d[..., 0] / d[..., 2] * W, d[..., 1] / d[..., 2] * H, d[..., 2]


def wave_range(lo, hi, origin, flip):                                # inclusive wave indices whose sub-sample range meets [lo, hi]
    if not flip:
        return int(max(0, np.ceil((lo + origin - 3.5) / 4))), int(min(wx - 1, np.floor((hi + origin) / 4)))
    return int(max(0, np.ceil((origin - 3.0 - hi) / 4))), int(min(wy - 1, np.floor((origin + 0.5 - lo) / 4)))


box_mask, tight_mask, n_huge = np.zeros((wy, wx), bool), np.zeros((wy, wx), bool), 0
fine_mask, wide_cnt, wide_rects, root_sizes = np.zeros((wy, wx), bool), np.zeros((wy, wx), np.int32), [], []
bxs = np.arange(wx)[None, :] * 4.0 - half_w                         # a wave's sub-samples span [x, x + 3.5] x [y - 3, y + 0.5]
bys = top - np.arange(wy)[:, None] * 4.0
for t, own in zip(pos, in_root):
    lo, hi = t.min(0) - PAD, t.max(0) + PAD
    corners = np.array([[(hi if (k >> j) & 1 else lo)[j] for j in range(3)] for k in range(8)])
    xd, yd, g = project(corners)
    if (g <= 0).any():
        box_mask[:] = True; tight_mask[:] = True; fine_mask[:] = True
        continue
    x0, x1 = wave_range(xd.min() - MARGIN, xd.max() + MARGIN, half_w, False)
    y0, y1 = wave_range(yd.min() - MARGIN, yd.max() + MARGIN, top, True)
    if x0 > x1 or y0 > y1:
        continue
    box_mask[y0:y1 + 1, x0:x1 + 1] = True
    n_w = (x1 - x0 + 1) * (y1 - y0 + 1)
    if own: root_sizes.append(n_w)
    whole_frame = x0 == 0 and y0 == 0 and x1 == wx - 1 and y1 == wy - 1
    if own and n_w >= WIDE_MIN_WAVES and n_w * WIDE_FRAME_SHARE >= wx * wy and not whole_frame and len(wide_rects) < MAX_WIDE:   # (list order here; the pass takes whichever boxes come first)
        wide_rects.append((x0, x1, y0, y1)); wide_cnt[y0:y1 + 1, x0:x1 + 1] += 1
    else:
        fine_mask[y0:y1 + 1, x0:x1 + 1] = True
    if (x1 - x0 + 1) * (y1 - y0 + 1) <= HUGE:
        tight_mask[y0:y1 + 1, x0:x1 + 1] = True
        continue
    # a huge box: per wave, the three edge functions of the projected vertices, each pushed outward by the projected pad plus the margin; a wave (a rectangle of
    # sub-samples) lies outside the padded triangle's hull if all four of its corners are outside ONE edge
    n_huge += 1
    vx, vy, vg = project(t)
    push = PAD * np.sqrt(3.0) * max(W, H) / vg.min() + MARGIN        # a pad-ball around a point at depth >= min(gamma) projects within this many sub-sample units
    sgn = np.sign((vx[1] - vx[0]) * (vy[2] - vy[0]) - (vy[1] - vy[0]) * (vx[2] - vx[0])) or 1.0
    inside = np.ones((y1 - y0 + 1, x1 - x0 + 1), bool)
    X0, X1 = bxs[:, x0:x1 + 1], bxs[:, x0:x1 + 1] + 3.5
    Y0, Y1 = bys[y0:y1 + 1] - 3.0, bys[y0:y1 + 1] + 0.5
    for i in range(3):
        ax, ay, bx, by = vx[i], vy[i], vx[(i + 1) % 3], vy[(i + 1) % 3]
        nx, ny = -(by - ay) * sgn, (bx - ax) * sgn                    # inward normal of edge a -> b
        ln = np.hypot(nx, ny) or 1.0
        f = lambda X, Y: ((X - ax) * nx + (Y - ay) * ny) / ln
        best = np.maximum(np.maximum(f(X0, Y0), f(X1, Y0)), np.maximum(f(X0, Y1), f(X1, Y1)))
        inside &= best >= -push
    tight_mask[y0:y1 + 1, x0:x1 + 1] |= inside
n = wx * wy
print(f"{os.path.basename(scene)} {W}x{H}: {len(pos)} triangles, {n} waves")
print(f"  box rule: {n - int(box_mask.sum())} waves proved empty = {100.0 * (n - box_mask.sum()) / n:.2f} %")
print(f"  with the triangle test for the {n_huge} boxes above {HUGE} waves: {n - int(tight_mask.sum())} = {100.0 * (n - tight_mask.sum()) / n:.2f} %"
      f"  (+{100.0 * (int(box_mask.sum()) - int(tight_mask.sum())) / n:.2f} points)")
simple = box_mask & ~fine_mask
covered, n_simple = int(box_mask.sum()), int(simple.sum())
rs = np.sort(np.asarray(root_sizes))[::-1]
print(f"  root's own list: {int(in_root.sum())} triangles; boxes of it covering >= 100 / 200 / 400 / 800 / 1600 waves: " + " / ".join(str(int((rs >= k).sum())) for k in (100, 200, 400, 800, 1600)))
print(f"  frame share: boxes of the root's list covering >= 1/512, 1/256, 1/128, 1/64 of the frame: " + " / ".join(str(int((rs * k >= wx * wy).sum())) for k in (512, 256, 128, 64)))
print(f"  wide boxes (>= {WIDE_MIN_WAVES} waves and 1/{WIDE_FRAME_SHARE} of the frame, root's list, at most {MAX_WIDE}): {len(wide_rects)}")
print(f"  simple waves: {n_simple} of {covered} covered = {100.0 * n_simple / max(covered, 1):.1f} %; wide boxes per simple wave: mean {wide_cnt[simple].mean() if n_simple else 0.0:.2f}, max {int(wide_cnt[simple].max()) if n_simple else 0}")
