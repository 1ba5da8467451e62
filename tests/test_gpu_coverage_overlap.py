"""The coverage pass beside the frame before it (csrc/frames.cpp: launch_whole_frame, take_cover_buffer; csrc/cover_pool.hpp): where the caller's stream is busy at
the call, the pass of a frame runs on the raytracer's side stream into one of two buffers per stream, and render_kernel waits for it behind an event.  What can
go wrong is ORDER: a mask read before it is filled, a mask overwritten under the kernel that reads it, a frame that gets the mask of the frame before or after.
So every case enqueues frames WITHOUT synchronising (a forced walk: nothing measures), with masks that differ from frame to frame, and compares every frame bit
for bit with the frame of a second raytracer with coverage=False in the same pose.

The scene is sparse and flat (no pow): a quad and three small triangles about 12 degrees to either side of the view axis.  The two poses share the creation eye
-- set_camera with a bit-equal eye is host work, no GPU call and no synchronisation -- and turn the view by 13 degrees to the right or to the left, so that the
geometry lies in the left half of the frame, then in the right half: the masks are near-complements, and a frame that ran with the other pose's mask has WHITE
holes where its geometry is.  test_poses_on_the_cpu holds the scene to that without a GPU.  72x40 has tiles_x = 9 and 136x72 has 17: no multiple of 8.

 (a) twelve frames alternating the poses on ONE stream; the last frame's mask against the rule restated (tests/coverage_checks.py);
 (b) two frame sizes on one stream (the buffers regrow while frames are queued);
 (c) three streams and the null stream in turn, sixteen frames;
 (d) set_triangles between two unsynchronised frames;
 (e) blocking and non-blocking calls mixed, and a launch on a stream that is idle again;
 (f) the default path once: three teapot frames at 1920x1080 back to back, no flag;
 (g) a raytracer destroyed with four frames in flight.
"""
import numpy as np
import pytest

import coverage_checks as cc
from bitwise import assert_same_bits
from gpu_checks import ORIGIN

ON = "always"              # RRT_FLAG_COVERAGE_ALWAYS: the frames here are small on purpose
WHITE = 0x00FFFFFF
VIEWPORT = (1.0, 1.0, 1.0)
FLAT = [dict(ka=(1, 1, 1), kd=(1, 1, 1), ks=(0, 0, 0), ns=-1.0, kr=0.0, tex=0, bump=-1)]          # no specular term, no reflection: no pow
TEX = [np.full((2, 2, 3), (200, 60, 20), np.uint8)]                                               # (no lighting brings its blue channel to 255: a hit is never WHITE)
PAD = 20.0 / 32768.0                                                                              # the index pad of the default root box
W, H = 72, 40
W2, H2 = 136, 72


def yawed(degrees):
    """The creation eye, the view turned about the y axis: positive turns it to the right, so that what lay ahead appears on the left."""
    a = np.radians(degrees)
    return dict(eye=ORIGIN, right=(float(np.cos(a)), 0.0, float(-np.sin(a))), up=(0.0, 1.0, 0.0), forward=(float(np.sin(a)), 0.0, float(np.cos(a))))


POSES = (yawed(13.0), yawed(-13.0))          # geometry in the left half, in the right half
AHEAD = dict(eye=ORIGIN, right=(1.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), forward=(0.0, 0.0, 1.0))


def triangles(shift=0.0):
    """A quad of two triangles at depth 10 (x in [-2.1, 2.1], y in [-1.5, 5.5]) and three small triangles at other depths in front of it, moved by `shift` in x."""
    pos = np.array([[(-2.1, -1.5, 0.0), (2.1, -1.5, 0.0), (2.1, 5.5, 0.0)],
                    [(-2.1, -1.5, 0.0), (2.1, 5.5, 0.0), (-2.1, 5.5, 0.2)],
                    [(-1.2, 4.0, -3.0), (-0.9, 4.1, -3.0), (-1.1, 4.4, -2.8)],
                    [(0.8, 0.2, -4.0), (1.1, 0.1, -4.2), (0.9, 0.6, -4.0)],
                    [(-0.2, 2.0, -5.0), (0.1, 2.0, -5.0), (0.0, 2.3, -5.1)]], np.float64)
    return pos + np.array([shift, 0.0, 0.0])


LEFT, RIGHT = -2.6, 2.6                       # (d): the scene in the left half of the creation pose's frame, then in the right half


def arrays(pos):
    n = len(pos)
    nrm = np.cross(pos[:, 1] - pos[:, 0], pos[:, 2] - pos[:, 0]); nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    return pos, np.zeros((n, 3, 3)), np.repeat(nrm[:, None], 3, 1), np.zeros(n, np.uint32)


def approx_boxes(pos):
    """(c, h) of the triangles' boxes padded by PAD, in fp32: close to the device's records, enough to judge the scene on the CPU."""
    lo, hi = pos.min(1) - PAD, pos.max(1) + PAD
    return ((lo + hi) * 0.5).astype(np.float32), ((hi - lo) * 0.5 * (1.0 + 2.0 ** -20)).astype(np.float32)


def restated_mask(w, h, cam, boxes):
    F = cc.frame_of(w, h, VIEWPORT, cam["right"], cam["up"], cam["forward"], cam["eye"])
    return cc.mask_of(F, cc.rects_of(F, *boxes) if isinstance(boxes, tuple) else cc.rects_of(F, boxes))


def assert_near_complements(masks, what):
    a, b = masks
    for k, m in enumerate(masks):
        assert (~m).sum() * 4 >= m.size and m.any(), f"{what}: pose {k} proves {int((~m).sum())} of {m.size} waves empty"
    assert (a != b).sum() * 4 >= a.size, f"{what}: the two masks differ in {int((a != b).sum())} of {a.size} bits"


def test_poses_on_the_cpu():
    """Each pose proves at least a quarter of the waves empty, and the masks of the two poses (and of the two scenes of (d)) differ in at least a quarter of the bits."""
    for w, h in ((W, H), (W2, H2)):
        assert ((w + 7) // 8) % 8 != 0
        assert_near_complements([restated_mask(w, h, cam, approx_boxes(triangles())) for cam in POSES], f"{w}x{h}, the two poses")
    assert_near_complements([restated_mask(W, H, AHEAD, approx_boxes(triangles(s))) for s in (LEFT, RIGHT)], "the two scenes of (d)")


# ------------------------------------------------------------------ the raytracers and the expected frames
@pytest.fixture(scope="module")
def sparse(rrt):
    """(SceneData, lights, expected): expected[(w, h, k)] is the frame of pose k from a raytracer with coverage=False; computed once, read-only."""
    sd = rrt.SceneData.from_arrays(*arrays(triangles()), FLAT, TEX)
    lights = rrt.default_lights()
    off = rrt.RayTracer(sd, lights, box_filter="bundle", coverage=False)
    expected = {}
    for k, cam in enumerate(POSES):
        off.set_camera(**cam)
        for w, h in ((W, H), (W2, H2)):
            expected[(w, h, k)] = off.render(w, h)
            expected[(w, h, k)].setflags(write=False)
            assert off.coverage_info()["state"] == "flag"
            body = expected[(w, h, k)][1:]
            half = body[:, :w // 2] if k == 0 else body[:, w // 2:]
            other = body[:, w // 2:] if k == 0 else body[:, :w // 2]
            assert (half != WHITE).sum() * 4 > half.size and (other == WHITE).all(), f"pose {k} at {w}x{h}: the geometry does not lie in its half of the frame"
    return sd, lights, expected


def frame_of(fb, w, h):
    return fb.cpu().numpy().view(np.uint32).reshape(h, w)


def framebuffers(sizes):
    import torch
    fbs = [torch.zeros(w * h, dtype=torch.int32, device="cuda") for w, h in sizes]
    torch.cuda.synchronize()
    return fbs


def assert_last_mask(rt, w, h, cam, what):
    want = restated_mask(w, h, cam, rt.buffer("tboxes"))
    got = rt.coverage_mask()
    assert got is not None and np.array_equal(got, want), f"{what}: the last frame's mask is not the rule's: {int((got != want).sum())} of {want.size} waves differ"
    return want


# ------------------------------------------------------------------ (a)
@pytest.mark.gpu
@pytest.mark.parametrize("pattern", ("alternating", "in pairs"))
def test_alternating_poses_on_one_stream(rrt, sparse, pattern):
    """Alternating: the neighbours of every frame have the other pose's mask.  In pairs (left, left, right, right, ...): the stream alternates between two buffers,
    so there the mask a buffer still holds from its last frame is the other pose's as well -- a frame that does not wait for its own mask shows holes."""
    import torch
    sd, lights, expected = sparse
    rt = rrt.RayTracer(sd, lights, box_filter="bundle", coverage=ON)
    stream = torch.cuda.Stream()
    n = 12
    pose_of = (lambda k: k % 2) if pattern == "alternating" else (lambda k: (k // 2) % 2)
    fbs = framebuffers([(W, H)] * n)
    states = []
    for k in range(n):
        rt.set_camera(**POSES[pose_of(k)])
        rt.render_into(fbs[k], W, H, stream=stream.cuda_stream)
        states.append(rt.coverage_info()["state"])
    torch.cuda.synchronize()
    assert states == ["on"] * n, states
    for k in range(n):
        assert_same_bits(frame_of(fbs[k], W, H), expected[(W, H, pose_of(k))], f"frame {k} of {n}, pose {pose_of(k)}")
    assert_last_mask(rt, W, H, POSES[pose_of(n - 1)], f"twelve frames, poses {pattern}")
    assert_near_complements([restated_mask(W, H, cam, rt.buffer("tboxes")) for cam in POSES], "the device's records")


# ------------------------------------------------------------------ (b)
@pytest.mark.gpu
def test_two_frame_sizes_on_one_stream(rrt, sparse):
    """Small, small, large, large, then alternating: the stream's two buffers are both made for the small frame first, and each grows while frames are queued."""
    import torch
    sd, lights, expected = sparse
    rt = rrt.RayTracer(sd, lights, box_filter="bundle", coverage=ON)
    stream = torch.cuda.Stream()
    sizes = [(W, H), (W, H), (W2, H2), (W2, H2)] + [(W, H), (W2, H2)] * 4
    pose_of = lambda k: (k // 2) % 2          # (in pairs: what a buffer holds from its last frame is the other pose's mask, and often the other size's)
    fbs = framebuffers(sizes)
    states = []
    for k, (w, h) in enumerate(sizes):
        rt.set_camera(**POSES[pose_of(k)])
        rt.render_into(fbs[k], w, h, stream=stream.cuda_stream)
        states.append(rt.coverage_info()["state"])
    torch.cuda.synchronize()
    assert states == ["on"] * len(sizes), states
    for k, (w, h) in enumerate(sizes):
        assert_same_bits(frame_of(fbs[k], w, h), expected[(w, h, pose_of(k))], f"frame {k}, {w}x{h}, pose {pose_of(k)}")
    k = len(sizes) - 1
    assert_last_mask(rt, *sizes[k], POSES[pose_of(k)], "two sizes on one stream")


# ------------------------------------------------------------------ (c)
@pytest.mark.gpu
def test_three_streams_and_the_null_stream(rrt, sparse):
    import torch
    sd, lights, expected = sparse
    rt = rrt.RayTracer(sd, lights, box_filter="bundle", coverage=ON)
    streams = [s.cuda_stream for s in (torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream())] + [0]
    n = 16
    pose_of = lambda k: (k % 2) ^ (0, 1, 1, 0)[k // 4]      # alternating within every round of the four streams; a stream's four frames see poses p, ~p, ~p, p, so
                                                            # that each of its two buffers holds the other pose's mask when it comes back
    fbs = framebuffers([(W, H)] * n)
    states = []
    for k in range(n):
        rt.set_camera(**POSES[pose_of(k)])
        rt.render_into(fbs[k], W, H, stream=streams[k % 4])
        states.append(rt.coverage_info()["state"])
    torch.cuda.synchronize()
    assert states == ["on"] * n, states       # four streams, two buffers each: the pool's eight
    for k in range(n):
        assert_same_bits(frame_of(fbs[k], W, H), expected[(W, H, pose_of(k))], f"frame {k} on stream {k % 4}, pose {pose_of(k)}")
    assert_last_mask(rt, W, H, POSES[pose_of(n - 1)], "four streams in turn")


# ------------------------------------------------------------------ (d)
@pytest.mark.gpu
def test_set_triangles_between_two_unsynchronised_frames(rrt):
    import torch
    lights = rrt.default_lights()
    old, new = arrays(triangles(LEFT)), arrays(triangles(RIGHT))
    want = [rrt.RayTracer.from_arrays(*a, FLAT, TEX, lights, box_filter="bundle", coverage=False).render(W, H) for a in (old, new)]
    body = [f[1:] for f in want]
    assert (body[0][:, W // 2:] == WHITE).all() and (body[1][:, :W // 2] == WHITE).all() and (body[0] != WHITE).any() and (body[1] != WHITE).any()
    rt = rrt.RayTracer.from_arrays(*old, FLAT, TEX, lights, box_filter="bundle", coverage=ON)
    stream = torch.cuda.Stream()
    fbs = framebuffers([(W, H)] * 3)
    rt.render_into(fbs[0], W, H, stream=stream.cuda_stream)      # (a frame in front, so that the next one finds its stream busy)
    rt.render_into(fbs[1], W, H, stream=stream.cuda_stream)
    rt.set_triangles(*new)
    rt.render_into(fbs[2], W, H, stream=stream.cuda_stream)
    assert rt.coverage_info()["state"] == "on"
    torch.cuda.synchronize()
    assert_same_bits(frame_of(fbs[2], W, H), want[1], "the frame after set_triangles")
    new_mask = assert_last_mask(rt, W, H, AHEAD, "the frame after set_triangles")
    assert not new_mask[:, :W // 8].any() and new_mask.any(), "the new scene's mask is set in the left half, or nowhere"
    for k in (0, 1):
        assert_same_bits(frame_of(fbs[k], W, H), want[0], f"frame {k} before set_triangles, read afterwards")


# ------------------------------------------------------------------ (e)
@pytest.mark.gpu
def test_blocking_and_non_blocking_calls_mixed(rrt, sparse):
    import torch
    sd, lights, expected = sparse
    rt = rrt.RayTracer(sd, lights, box_filter="bundle", coverage=ON)
    fbs = framebuffers([(W, H)] * 5)
    states = []

    def launch(k, pose):
        rt.set_camera(**POSES[pose])
        rt.render_into(fbs[k], W, H)                             # the current torch stream: the null stream
        states.append(rt.coverage_info()["state"])

    launch(0, 0); launch(1, 1)
    rt.set_camera(**POSES[0])
    blocking = rt.render(W, H)                                   # blocking, on the raytracer's own stream, with two frames in flight on the null stream
    states.append(rt.coverage_info()["state"])
    launch(2, 1); launch(3, 0)
    torch.cuda.synchronize()
    launch(4, 1)                                                 # its stream is idle: the pass goes in front of render_kernel on that stream
    assert_last_mask(rt, W, H, POSES[1], "a launch on an idle stream")
    torch.cuda.synchronize()
    assert states == ["on"] * 6, states
    assert_same_bits(blocking, expected[(W, H, 0)], "the blocking frame between non-blocking launches")
    for k, pose in enumerate((0, 1, 1, 0, 1)):
        assert_same_bits(frame_of(fbs[k], W, H), expected[(W, H, pose)], f"non-blocking frame {k}, pose {pose}")


# ------------------------------------------------------------------ (f)
@pytest.mark.gpu
def test_default_path_three_frames_back_to_back(rrt, teapot):
    import torch
    w, h = 1920, 1080
    lights = rrt.default_lights()
    rt, off = rrt.RayTracer(teapot, lights, box_filter="bundle"), rrt.RayTracer(teapot, lights, box_filter="bundle", coverage=False)
    fbs = framebuffers([(w, h)] * 4)
    off.render_into(fbs[3], w, h)
    torch.cuda.synchronize()
    states = []
    for k in range(3):
        rt.render_into(fbs[k], w, h)
        states.append(rt.coverage_info()["state"])
    torch.cuda.synchronize()
    assert states == ["on"] * 3 and off.coverage_info()["state"] == "flag", states
    assert int((fbs[3] != WHITE).sum()) > w * h // 4
    for k in range(3):
        assert torch.equal(fbs[k], fbs[3]), f"frame {k}: {int((fbs[k] != fbs[3]).sum())} pixels differ from the coverage=False frame"


# ------------------------------------------------------------------ (g)
@pytest.mark.gpu
def test_destroy_with_frames_in_flight(rrt, teapot):
    import torch
    w, h = 1920, 1080
    lights = rrt.default_lights()
    fbs = framebuffers([(w, h)] * 6)
    off = rrt.RayTracer(teapot, lights, box_filter="bundle", coverage=False)
    off.render_into(fbs[4], w, h)
    rt = rrt.RayTracer(teapot, lights, box_filter="bundle")
    for k in range(4):
        rt.render_into(fbs[k], w, h)
    assert rt.coverage_info()["state"] == "on"
    del rt                                                        # rrt_raytracer_destroy with four frames in flight
    other = rrt.RayTracer(teapot, lights, box_filter="bundle")
    other.render_into(fbs[5], w, h)
    assert other.coverage_info()["state"] == "on"
    torch.cuda.synchronize()
    for k in (0, 1, 2, 3, 5):
        assert torch.equal(fbs[k], fbs[4]), f"frame {k}: {int((fbs[k] != fbs[4]).sum())} pixels differ from the coverage=False frame"
