// Stand-alone host check of csrc/coverage_rule.hpp (tests/test_coverage_rule.py builds and runs it; never linked into the library).
//   coverage_rule_model N     sweeps about N (box, camera, ray) tuples and prints one line of counts; exit status 0 unless the program itself is broken.
//   coverage_rule_model --pairs IN OUT     (second mode; "-" is stdin / stdout) reads (frame, box) pairs in binary and writes what the header makes of each:
//       in, 152 bytes:  uint32 width, height; double x_scale, y_scale, z_value, right[3], up[3], forward[3], eye[3]; float c[3], h[3]
//       out, 136 bytes: int32 ok (coverage_frame), bx0, bx1, by0, by1 (coverage_rect), whole (coverage_is_whole_frame); uint32 tiles_x, tiles_y;
//                       double inv[9], kx, ky, half_w, top          (everything after ok is 0 where ok is 0)
//     tests/test_coverage_restatement.py requires every field to equal tests/coverage_checks.py's.
// For every tuple: the ray is formed exactly as render_kernel forms the primary ray of a sub-sample; wherever a slab test of that ray against the box [c - h, c + h]
// says "meets" -- in f64 or in long double -- the rule must have marked the sub-sample's wave.  A failure is counted, not fatal: the test that builds this program
// with the margin negated expects failures.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "coverage_rule.hpp"

using namespace rrt;

namespace {

struct Rng {
    uint64_t s;
    uint64_t next() { s += 0x9E3779B97F4A7C15ull; uint64_t z = s; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
    double uni() { return (double)(next() >> 11) * 0x1p-53; }                      // [0, 1)
    double range(double a, double b) { return a + (b - a) * uni(); }
    uint32_t below(uint32_t n) { return (uint32_t)(next() % n); }
};

struct Camera { uint32_t W, H; double x_scale, y_scale, z_value, right[3], up[3], forward[3], eye[3]; };

// the primary ray of sub-sample `sub` of pixel (px, py): render.hip, render_kernel -- five operations per component, each rounded on its own
void primary_direction(const Camera& C, uint32_t px, uint32_t py, uint32_t sub, double d[3]) {
    const int32_t W = (int32_t)C.W, H = (int32_t)C.H;
    const int32_t x = (int32_t)px - W / 2, y = (H - H / 2) - (int32_t)py;
    const double xd = (sub & 1u) ? ((double)x + 0.5) : (double)x, yd = (sub & 2u) ? ((double)y + 0.5) : (double)y;
    const double sa = xd * C.x_scale, sb = yd * C.y_scale, sc = C.z_value;
    for (int k = 0; k < 3; k++) d[k] = (C.right[k] * sa + C.up[k] * sb) + C.forward[k] * sc;
}
bool traced(const Camera& C, uint32_t px, uint32_t py) {
    const int32_t W = (int32_t)C.W, H = (int32_t)C.H;
    return (int32_t)px < 2 * (W / 2) && (int32_t)py >= H - 2 * (H / 2) + 1 && (int32_t)py < H;
}

// does the ray o + t d, t >= 0, meet the box [c - h, c + h]?
template <class T> bool slab(const double o[3], const double d[3], const float c[3], const float h[3]) {
    T t0 = 0, t1 = INFINITY;
    for (int k = 0; k < 3; k++) {
        const T lo = (T)c[k] - (T)h[k], hi = (T)c[k] + (T)h[k];
        if (d[k] == 0.0) { if ((T)o[k] < lo || (T)o[k] > hi) return false; continue; }
        T a = (lo - (T)o[k]) / (T)d[k], b = (hi - (T)o[k]) / (T)d[k];
        if (a > b) { const T s = a; a = b; b = s; }
        t0 = a > t0 ? a : t0; t1 = b < t1 ? b : t1;
    }
    return t0 <= t1;
}

const uint32_t kSizes[][2] = {{1, 1}, {2, 2}, {3, 5}, {7, 1}, {1, 7}, {37, 23}, {64, 48}, {64, 32}, {96, 64}, {1920, 1080}, {3840, 2160}, {641, 479}};

void rotate(Rng& R, double right[3], double up[3], double forward[3]) {   // a random orthonormal basis (to rounding): Gram-Schmidt of random vectors
    double a[3], b[3];
    for (;;) {
        for (int k = 0; k < 3; k++) { a[k] = R.range(-1, 1); b[k] = R.range(-1, 1); }
        const double la = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
        if (la < 0.1) continue;
        for (int k = 0; k < 3; k++) a[k] /= la;
        const double ab = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
        for (int k = 0; k < 3; k++) b[k] -= ab * a[k];
        const double lb = std::sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
        if (lb < 0.1) continue;
        for (int k = 0; k < 3; k++) b[k] /= lb;
        break;
    }
    for (int k = 0; k < 3; k++) { forward[k] = a[k]; right[k] = b[k]; }
    up[0] = forward[1] * right[2] - forward[2] * right[1]; up[1] = forward[2] * right[0] - forward[0] * right[2]; up[2] = forward[0] * right[1] - forward[1] * right[0];
}

Camera random_camera(Rng& R, int mode) {
    Camera C{};
    const uint32_t* s = kSizes[R.below(sizeof kSizes / sizeof kSizes[0])];
    C.W = s[0]; C.H = s[1];
    const double id[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int k = 0; k < 3; k++) { C.right[k] = id[0][k]; C.up[k] = id[1][k]; C.forward[k] = id[2][k]; }
    if (mode >= 1) rotate(R, C.right, C.up, C.forward);
    if (mode >= 2) {                                                        // not orthonormal: axes of different lengths, sheared into each other
        const double sr = R.range(0.5, 2.0), su = R.range(0.5, 2.0), sf = R.range(0.5, 2.0), sh1 = R.range(-0.4, 0.4), sh2 = R.range(-0.4, 0.4);
        for (int k = 0; k < 3; k++) { const double r = C.right[k] * sr, u = C.up[k] * su + sh1 * C.right[k], f = C.forward[k] * sf + sh2 * C.up[k]; C.right[k] = r; C.up[k] = u; C.forward[k] = f; }
    }
    const double vw = mode ? R.range(0.5, 2.0) : 1.0, vh = mode ? R.range(0.5, 2.0) : 1.0;
    C.x_scale = vw / (double)C.W; C.y_scale = vh / (double)C.H; C.z_value = mode ? R.range(0.5, 2.0) : 1.0;
    for (int k = 0; k < 3; k++) C.eye[k] = mode ? R.range(-10, 10) : (double)((int)R.below(9) - 4);
    return C;
}

struct Counts { uint64_t tuples = 0, meets = 0, exact_meets = 0, failures = 0, whole = 0, partial = 0, cameras_off = 0, straddle = 0, zero_extent = 0, loose = 0; };

// one ray against one box: the check itself
void check(const Camera& C, const CoverageFrame& F, const CoverageRect& r, const float c[3], const float h[3], uint32_t px, uint32_t py, uint32_t sub, Counts& n, bool exact) {
    if (px >= C.W || py >= C.H || !traced(C, px, py)) return;
    double d[3];
    primary_direction(C, px, py, sub, d);
    n.tuples++;
    if (!(slab<double>(C.eye, d, c, h) || slab<long double>(C.eye, d, c, h))) return;
    n.meets++; n.exact_meets += exact;
    const int32_t bx = (int32_t)(px / 4u), by = (int32_t)(py / 4u);
    if (bx >= r.bx0 && bx <= r.bx1 && by >= r.by0 && by <= r.by1) return;
    if (n.failures++ < 5)
        fprintf(stderr, "UNMARKED: frame %ux%u pixel (%u, %u) sub %u wave (%d, %d), rect x [%d, %d] y [%d, %d], box c (%.9g %.9g %.9g) h (%.9g %.9g %.9g) eye (%.17g %.17g %.17g)\n",
                C.W, C.H, px, py, sub, bx, by, r.bx0, r.bx1, r.by0, r.by1, c[0], c[1], c[2], h[0], h[1], h[2], C.eye[0], C.eye[1], C.eye[2]);
    (void)F;
}

// the sub-samples around the point (xd, yd) of the frame's plane, and a few further away
void check_around(Rng& R, const Camera& C, const CoverageFrame& F, const CoverageRect& r, const float c[3], const float h[3], double xd, double yd, Counts& n) {
    if (!(std::fabs(xd) < 1e7 && std::fabs(yd) < 1e7)) return;
    const int32_t W = (int32_t)C.W, H = (int32_t)C.H;
    const double fx = std::floor(xd * 2.0) / 2.0, fy = std::floor(yd * 2.0) / 2.0;            // the grid of sub-samples has pitch 0.5
    for (int i = -1; i <= 2; i++) for (int j = -1; j <= 2; j++) {
        const double sx = fx + 0.5 * i, sy = fy + 0.5 * j;
        const double x = std::floor(sx), y = std::floor(sy);
        const int64_t px = (int64_t)x + W / 2, py = (int64_t)(H - H / 2) - (int64_t)y;
        if (px < 0 || py < 0 || px >= W || py >= H) continue;
        check(C, F, r, c, h, (uint32_t)px, (uint32_t)py, (sx != x ? 1u : 0u) | (sy != y ? 2u : 0u), n, false);
    }
    for (int i = 0; i < 2; i++) check(C, F, r, c, h, R.below(C.W), R.below(C.H), R.below(4), n, false);
}

// A: random boxes of every extent around a point on a random primary ray, aimed at from the sub-samples around the projections of their corners, centre and inside
void sweep_random(Rng& R, uint64_t boxes, Counts& n) {
    for (uint64_t i = 0; i < boxes; i++) {
        const Camera C = random_camera(R, (int)(i % 3));
        CoverageFrame F;
        if (!coverage_frame(F, C.W, C.H, C.x_scale, C.y_scale, C.z_value, C.right, C.up, C.forward, C.eye)) { n.cameras_off++; continue; }
        double d[3];
        // a sub-sample inside the frame, at its edge or (one pixel) beyond it
        const uint32_t edge = R.below(4);
        uint32_t px = edge == 0 ? 0u : edge == 1 ? C.W - 1u : R.below(C.W), py = edge == 2 ? C.H - 1u : edge == 3 ? (C.H > 1 ? 1u : 0u) : R.below(C.H);
        primary_direction(C, px, py, R.below(4), d);
        const double t = std::exp(R.range(std::log(0.05), std::log(200.0)));
        float c[3], h[3];
        const int kind = (int)R.below(6);                                  // 0: a point; 1: flat; 2: tiny; 3: small; 4: large; 5: around the eye plane
        for (int k = 0; k < 3; k++) {
            c[k] = (float)(C.eye[k] + t * d[k] + (kind >= 3 ? R.range(-1, 1) * t * 0.05 : 0.0));
            const double e = kind == 0 ? 0.0 : kind == 1 ? (R.below(2) ? 0.0 : R.range(0, 0.3) * t) : kind == 2 ? std::ldexp(R.uni(), -20) * t
                           : kind == 3 ? R.range(0, 0.05) * t : kind == 4 ? R.range(0, 2.0) * t : R.range(0.5, 1.5) * t * std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
            h[k] = (float)e;
        }
        if (kind == 0) n.zero_extent++;
        const CoverageRect r = coverage_rect(F, c, h);
        const bool whole = coverage_is_whole_frame(F, r) && C.W * C.H > 64u;
        n.whole += whole; n.partial += !whole;
        bool behind = false;
        double lo_x = HUGE_VAL, hi_x = -HUGE_VAL, lo_y = HUGE_VAL, hi_y = -HUGE_VAL;
        for (int k = 0; k <= 9; k++) {                                     // the eight corners, the centre, a point inside
            double P[3];
            for (int j = 0; j < 3; j++) P[j] = (double)c[j] + (k < 8 ? ((k >> j) & 1 ? 1.0 : -1.0) : k == 8 ? 0.0 : R.range(-1, 1)) * (double)h[j];
            long double abg[3];
            for (int a = 0; a < 3; a++) { abg[a] = 0; for (int j = 0; j < 3; j++) abg[a] += (long double)F.inv[a][j] * ((long double)P[j] - (long double)C.eye[j]); }
            if (!(abg[2] > 0)) { behind = true; continue; }
            const double xd = (double)(abg[0] / abg[2] * F.kx), yd = (double)(abg[1] / abg[2] * F.ky);
            if (k < 8) { lo_x = std::fmin(lo_x, xd); hi_x = std::fmax(hi_x, xd); lo_y = std::fmin(lo_y, yd); hi_y = std::fmax(hi_y, yd); }
            check_around(R, C, F, r, c, h, xd, yd, n);
        }
        n.straddle += behind;
        if (behind && !coverage_is_whole_frame(F, r)) { if (n.failures++ < 5) fprintf(stderr, "a box with a corner behind the eye must mark the whole frame\n"); }
        // not looser than its own statement: the rectangle of a box in front of the eye is the corners' bounding rectangle plus at most one wave on each side
        if (!behind && std::fabs(lo_x) < 1e6 && std::fabs(hi_x) < 1e6 && std::fabs(lo_y) < 1e6 && std::fabs(hi_y) < 1e6 && r.bx0 <= r.bx1 && r.by0 <= r.by1) {
            const double waves_x = (hi_x - lo_x) / 4.0 + 3.0, waves_y = (hi_y - lo_y) / 4.0 + 3.0;
            if ((double)(r.bx1 - r.bx0 + 1) > waves_x || (double)(r.by1 - r.by0 + 1) > waves_y) { n.loose++; if (n.failures++ < 5) fprintf(stderr, "rectangle wider than the projection allows\n"); }
        }
    }
}

// B: exact cases.  Identity basis, power-of-two frame, integer eye: every number below is exact in f64 and in fp32, so "meets" holds with equality.
//  * a box of zero extent at the point  eye + 4 dir  of a sub-sample: its ray meets it, and its wave must be marked (a negated margin gives an empty rectangle);
//  * a box whose corner lies on the ray of a sub-sample at the EDGE of a wave (xd = 4 bx - W/2 or 4 bx + 3.5 - W/2, likewise yd) and that extends away from
//    the wave: the wave touches the rectangle in that one point.
void sweep_exact(Rng& R, uint64_t boxes, Counts& n) {
    for (uint64_t i = 0; i < boxes; i++) {
        Camera C = random_camera(R, 0);
        C.W = 64; C.H = R.below(2) ? 32 : 64; C.x_scale = 1.0 / C.W; C.y_scale = 1.0 / C.H;
        CoverageFrame F;
        if (!coverage_frame(F, C.W, C.H, C.x_scale, C.y_scale, C.z_value, C.right, C.up, C.forward, C.eye)) { n.failures++; continue; }
        const bool corner = (i & 1) != 0;
        const uint32_t bx = R.below(C.W / 4), by = R.below(C.H / 4);
        const bool at_right = R.below(2), at_bottom = R.below(2);
        // the wave's extreme sub-sample in x and y (corner case), or any of its 64 (point case)
        const uint32_t px = 4 * bx + (corner ? (at_right ? 3u : 0u) : R.below(4)), py = 4 * by + (corner ? (at_bottom ? 3u : 0u) : R.below(4));
        const uint32_t sub = corner ? ((at_right ? 1u : 0u) | (at_bottom ? 0u : 2u)) : R.below(4);      // (+0.5 in x is to the right; +0.5 in y is UP: towards smaller py)
        if (!traced(C, px, py)) continue;
        double d[3];
        primary_direction(C, px, py, sub, d);
        float c[3], h[3];
        for (int k = 0; k < 3; k++) { c[k] = (float)(C.eye[k] + 4.0 * d[k]); h[k] = 0.0f; }
        if (corner) {                                                      // the point becomes the corner of a box that leaves the wave: right / left of it, below / above it
            const float e = 0.25f;
            h[0] = e; c[0] += at_right ? e : -e;
            h[1] = e; c[1] += at_bottom ? -e : e;                            // (scene y grows upwards, py downwards)
        }
        const CoverageRect r = coverage_rect(F, c, h);
        check(C, F, r, c, h, px, py, sub, n, true);
    }
}

struct PairIn { uint32_t width, height; double x_scale, y_scale, z_value, right[3], up[3], forward[3], eye[3]; float c[3], h[3]; };
struct PairOut { int32_t ok, bx0, bx1, by0, by1, whole; uint32_t tiles_x, tiles_y; double inv[9], kx, ky, half_w, top; };
static_assert(sizeof(PairIn) == 152 && sizeof(PairOut) == 136, "the record layouts tests/test_coverage_restatement.py reads and writes");

int pairs_mode(const char* in_name, const char* out_name) {
    FILE* in = strcmp(in_name, "-") ? fopen(in_name, "rb") : stdin;
    FILE* out = strcmp(out_name, "-") ? fopen(out_name, "wb") : stdout;
    if (!in || !out) { fprintf(stderr, "cannot open %s or %s\n", in_name, out_name); return 2; }
    PairIn p;
    uint64_t n = 0;
    while (fread(&p, sizeof p, 1, in) == 1) {
        PairOut o;
        memset(&o, 0, sizeof o);
        CoverageFrame F;
        if (coverage_frame(F, p.width, p.height, p.x_scale, p.y_scale, p.z_value, p.right, p.up, p.forward, p.eye)) {
            const CoverageRect r = coverage_rect(F, p.c, p.h);
            o.ok = 1; o.bx0 = r.bx0; o.bx1 = r.bx1; o.by0 = r.by0; o.by1 = r.by1; o.whole = coverage_is_whole_frame(F, r) ? 1 : 0;
            o.tiles_x = F.tiles_x; o.tiles_y = F.tiles_y;
            for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) o.inv[3 * i + j] = F.inv[i][j];
            o.kx = F.kx; o.ky = F.ky; o.half_w = F.half_w; o.top = F.top;
        }
        if (fwrite(&o, sizeof o, 1, out) != 1) { fprintf(stderr, "short write\n"); return 2; }
        n++;
    }
    if (out != stdout) fclose(out); else fflush(out);
    if (in != stdin) fclose(in);
    fprintf(stderr, "pairs=%llu\n", (unsigned long long)n);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "--pairs")) return pairs_mode(argv[2], argv[3]);
    const uint64_t N = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1000000ull;
    Rng R{0x5EEDC0DEull};
    Counts n;
    // the wave index is render_kernel's block index of a whole frame: tile-major, then the quadrant
    for (uint32_t tiles_x : {1u, 3u, 8u, 240u}) for (uint32_t py = 0; py < 40; py++) for (uint32_t px = 0; px < 8 * tiles_x; px++) {
        const uint32_t tile = (py / 8) * tiles_x + px / 8, quad = ((py % 8) / 4) * 2 + (px % 8) / 4;
        if (coverage_wave_index(tiles_x, px / 4, py / 4) != tile * 4 + quad) n.failures++;
    }
    // frames the rule must refuse
    {
        CoverageFrame F; const double e[3] = {0, 2, -10}, X[3] = {1, 0, 0}, Y[3] = {0, 1, 0}, Z[3] = {0, 0, 1}, nan3[3] = {NAN, 0, 0}, flat[3] = {1, 1e-9, 0}, big[3] = {0, 0, 1000.0};
        if (!coverage_frame(F, 64, 48, 1.0 / 64, 1.0 / 48, 1.0, X, Y, Z, e)) n.failures++;
        if (coverage_frame(F, 64, 48, 1.0 / 64, 1.0 / 48, 1.0, X, X, Z, e)) n.failures++;        // singular
        if (coverage_frame(F, 64, 48, 1.0 / 64, 1.0 / 48, 1.0, X, flat, Z, e)) n.failures++;     // nearly singular
        if (coverage_frame(F, 64, 48, 1.0 / 64, 1.0 / 48, 1.0, X, Y, big, e)) n.failures++;      // condition 1000
        if (coverage_frame(F, 64, 48, 1.0 / 64, 1.0 / 48, 1.0, nan3, Y, Z, e)) n.failures++;
        if (coverage_frame(F, 64, 48, 1.0 / 64, 1.0 / 48, 1.0, X, Y, Z, nan3)) n.failures++;
        if (coverage_frame(F, 64, 48, 1.0 / 64, 1.0 / 48, 0.0, X, Y, Z, e)) n.failures++;        // viewport depth 0
        if (coverage_frame(F, 64, 48, 1.0 / 64, 1.0 / 48, -1.0, X, Y, Z, e)) n.failures++;
        if (coverage_frame(F, 64, 48, 0.0, 1.0 / 48, 1.0, X, Y, Z, e)) n.failures++;             // z_value / x_scale is not finite
        // boxes the rule must treat as "everything" or "nothing"
        if (!coverage_frame(F, 64, 48, 1.0 / 64, 1.0 / 48, 1.0, X, Y, Z, e)) n.failures++;
        const float c0[3] = {0, 0, 0}, never[3] = {-3.4028235e38f, -3.4028235e38f, -3.4028235e38f}, always[3] = {3.4028235e38f, 3.4028235e38f, 3.4028235e38f}, bad[3] = {NAN, 1, 1}, inf3[3] = {INFINITY, 1, 1};
        CoverageRect r = coverage_rect(F, c0, never);
        if (r.bx0 <= r.bx1 && r.by0 <= r.by1) n.failures++;
        if (!coverage_is_whole_frame(F, coverage_rect(F, c0, always))) n.failures++;
        if (!coverage_is_whole_frame(F, coverage_rect(F, c0, bad))) n.failures++;
        if (!coverage_is_whole_frame(F, coverage_rect(F, bad, c0))) n.failures++;
        if (!coverage_is_whole_frame(F, coverage_rect(F, c0, inf3))) n.failures++;
        // an unbounded record (c = 0, h = FLT_MAX along an axis) seen from an eye far beyond fp32's range: the whole frame, not the few waves around the origin's direction
        const double far_eye[3] = {0, 0x1p181, -0x1p183};
        if (!coverage_frame(F, 96, 72, 1.0 / 96, 1.0 / 72, 1.0, X, Y, Z, far_eye)) n.failures++;
        for (int k = 0; k < 3; k++) {
            float hk[3] = {1.0f, 1.0f, 1.0f}; hk[k] = 3.4028235e38f;
            if (!coverage_is_whole_frame(F, coverage_rect(F, c0, hk))) n.failures++;
        }
        const float nearly[3] = {3.4028233e38f, 3.4028233e38f, 3.4028233e38f};       // the largest finite extent below the mark is a length
        if (coverage_is_whole_frame(F, coverage_rect(F, c0, nearly))) n.failures++;
    }
    const uint64_t setup_failures = n.failures;
    sweep_exact(R, N / 16 + 1000, n);
    sweep_random(R, N / 80 + 1000, n);                                     // (each box is aimed at by about 170 rays)
    printf("tuples=%llu meets=%llu exact_meets=%llu whole=%llu partial=%llu straddle=%llu zero_extent=%llu cameras_off=%llu loose=%llu setup_failures=%llu failures=%llu\n",
           (unsigned long long)n.tuples, (unsigned long long)n.meets, (unsigned long long)n.exact_meets, (unsigned long long)n.whole, (unsigned long long)n.partial,
           (unsigned long long)n.straddle, (unsigned long long)n.zero_extent, (unsigned long long)n.cameras_off, (unsigned long long)n.loose, (unsigned long long)setup_failures,
           (unsigned long long)n.failures);
    return 0;
}
