"""The placements of tests/test_gpu_scene_placement.py and tests/test_gpu_coverage_poses.py: a scene mapped with p' = p s + shift, computed once in f64, and the
root box it is given.  The table of tests/test_gpu_scene_placement.py's docstring says which regime each one reaches.

Plain module, not a test module.  It holds no fixtures.
"""
import numpy as np

from gpu_checks import ROOT_BOX, PlainLight


class Placement:
    def __init__(self, pid, s=1.0, shift=(0.0, 0.0, 0.0), root=None):
        self.id, self.s, self.shift = pid, float(s), np.asarray(shift, np.float64)
        self.box = tuple(float(v) for v in self.pt(np.asarray(ROOT_BOX).reshape(3, 2).T).T.reshape(6))   # the reference's +-20 cube, mapped
        self.root = self.box if root is None else tuple(float(v) for v in root)
        self.mag = max(abs(v) for v in self.root)                 # scene_magnitude
        self.pad = self.mag / 32768.0
        self.offset = 1e-4 * self.s                               # surface_offset
        self.pow2 = not self.shift.any() and np.frexp(self.s)[0] == 0.5 and root is None

    def pt(self, p):
        """The map of points [..., 3]: one multiplication and one addition in f64."""
        return np.asarray(p, np.float64) * self.s + self.shift

    def lights(self, lights):
        """Point lights' positions are mapped; Ambient and Directional lights stay."""
        return [PlainLight(l.kind, l.intensity, tuple(self.pt((l.v.x, l.v.y, l.v.z))) if l.kind == 1 else (l.v.x, l.v.y, l.v.z)) for l in lights]

    def arrays(self, A):
        return dict(A, pos=self.pt(A["pos"]), root=self.root)


PLACEMENTS = {p.id: p for p in (
    Placement("small_pow2", 2.0 ** -10), Placement("small_dec", 1e-3), Placement("near_eps", 2.0 ** -18), Placement("large", 2.0 ** 40),
    Placement("f32_denormal_scale", 2.0 ** 120), Placement("f32_overflow", 2.0 ** 122), Placement("a_beyond_1e100", 2.0 ** 180),
    Placement("bounds_not_plain", 2.0 ** 200), Placement("shifted", 1.0, (1000.3, -517.7, 333.1)), Placement("scaled_shifted", 0.37, (-55.5, 7.25, 90.1)),
    Placement("far_shift", 1.0, (1e9, 1e9, -1e9)), Placement("anisotropic", root=(-20.1, 19.7, -3.3, 14.9, -12.7, 28.3)),
    Placement("cutting", root=(-2.9, 6.3, -0.45, 7.7, -6.1, 3.2)))}
