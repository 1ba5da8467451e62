// coverage_rule.hpp -- which 4x4-pixel waves of a whole frame can a padded box reach?  (coverage.hip: coverage_kernel; render.hip: render_kernel;
// DESIGN.md section 4, "coverage pass".)  Plain arithmetic, the same text for host and device, so that a stand-alone host program can check it against
// slab tests (tests/test_coverage_rule.py).
//
// THE FRAME.  render_kernel gives sub-sample (xd, yd) of a frame the direction  right*(xd*x_scale) + up*(yd*y_scale) + forward*z_value  from the eye, with
// xd = x or x + 0.5, x = px - W/2, and yd = y or y + 0.5, y = (H - H/2) - py.  Wave (bx, by) holds the pixels px in [4 bx, 4 bx + 3], py in [4 by, 4 by + 3]:
// its sub-samples span  xd in [4 bx - W/2, 4 bx + 3.5 - W/2],  yd in [(H - H/2) - 4 by - 3, (H - H/2) - 4 by + 0.5].
//
// THE RULE.  For a corner P of the box, (alpha, beta, gamma) = inv * (P - eye) are its coordinates in the view basis (inv: the inverse of the matrix
// whose columns are right, up, forward, taken once per launch on the host).  The ray from the eye through P is the one with
//     xd = (alpha / gamma) * kx,  kx = z_value / x_scale;      yd = (beta / gamma) * ky,  ky = z_value / y_scale,
// provided gamma > 0 and z_value > 0 (the ray parameter of P is gamma / z_value).  A box with a corner whose gamma is not certainly positive reaches
// the WHOLE frame (no clipping).  Otherwise the box reaches the waves whose sub-sample range meets the bounding rectangle of its eight (xd, yd),
// widened outward by the margin below.
//
// SOUNDNESS.  A box is convex, so the set of (xd, yd) whose rays meet it is the central projection of the box onto the plane gamma = z_value.  With
// every corner in front of the eye that projection is the convex hull of the corners' projections, which lies inside their bounding rectangle.  A ray
// whose (xd, yd) lies outside the rectangle of every slot's box meets no padded triangle box: the filters of the index drop every (ray, triangle) pair
// of it, and the index's own exactness argument ("exactness of the index, and its guard") says the reference's walk accepts none
// of them either.  The walk returns None and the sub-sample is WHITE.
//
// THE MARGIN.  Two sources of error separate the computed (xd, yd) from the exact ones.
//  (a) The coordinates.  inv comes from coverage_frame below, which accepts a basis only if  max |inv * M - I| <= 2^-43  and  |M|_inf |inv|_inf <= 256
//      (so the residual itself is computed to about 256 * 3 * 2^-53 < 2^-43).  The exact coordinates of d = P - eye are then the computed ones to within
//      E = kCoordRel * (s_a + s_b + s_g),  s_i = sum_j |inv_ij| |d_j|,  kCoordRel = 1e-12: the residual contributes at most 3 * 2^-42 = 6.9e-13 of
//      max(s), the rounding of the three products and two sums of a row 4 * 2^-53 of s_i, the rounding of P = c +- h and d = P - eye another 2^-52 each.
//      With g_lo = gamma - E > 0 the exact gamma is positive and
//          |alpha/gamma - alpha'/gamma'| = |alpha (gamma' - gamma) + gamma (alpha - alpha')| / (gamma gamma') <= (|alpha/gamma| E + E) / g_lo,
//      no first-order step.  The margin takes twice that, times |kx|.  For an orthonormal basis at 1920 pixels this is about 1e-8 pixel.
//  (b) Everything else -- the reciprocal of gamma and the product with it that stand for the quotient, the product with kx, the sums that turn a rectangle into wave indices, and the 2^-53-relative difference between
//      the ideal ray of a sub-sample and the direction render_kernel rounds five times: 1e-6 pixel plus 1e-9 of |xd|.  The operations involved are a
//      handful of f64 roundings (1e-15 relative), so this is nine orders above what it covers for a frame a million pixels wide, and still above it
//      at the largest width the library accepts (2^31).
// The real safety is neither: it is the pad of the box itself (2^-15 of the scene's magnitude), which is what makes "the ray misses the box" imply
// "the reference finds no hit".  The margin only has to keep the rule from being LESS careful than an exact projection of that box.
// UNBOUNDED RECORDS.  A half-extent of FLT_MAX is not a length: it is what the index writes, with c = 0, for an axis along which a padded bound left fp32's range
// (clusters.cpp and scene_build.hip: to_centre_half), and the filters read it as "always hit".  Taken as the box [-FLT_MAX, FLT_MAX] it does not contain a
// triangle of a scene whose coordinates lie beyond FLT_MAX (a root box scaled by 2^180: the eye is at 1e55, and the "box" projects onto a few waves around the
// direction of the origin -- tests/test_gpu_coverage_poses.py found 4092 of 6912 pixels WHITE that are not).  Such a box reaches the whole frame.
// RRT_COVERAGE_MARGIN_SIGN exists for the model test alone: built with -1 the rule must fail the sweep.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define RRT_COV_HD __host__ __device__
#else
#define RRT_COV_HD
#endif
#ifndef RRT_COVERAGE_MARGIN_SIGN
#define RRT_COVERAGE_MARGIN_SIGN 1.0
#endif

namespace rrt {

constexpr double kCoverCoordRel = 1e-12, kCoverAbsPix = 1e-6, kCoverRelPix = 1e-9;
constexpr double kCoverMaxResidual = 0x1p-43, kCoverMaxCond = 256.0;

// What the rule reads of a frame.  Filled by coverage_frame; passed to coverage_kernel by value.
struct CoverageFrame {
    double inv[3][3];            // (alpha, beta, gamma) = inv * (P - eye)
    double eye[3];
    double kx, ky;               // z_value / x_scale, z_value / y_scale
    double half_w, top;          // W/2 and H - H/2 (integer division), as doubles
    uint32_t tiles_x, tiles_y;   // 8x8-pixel tiles of the frame; waves_x = 2 tiles_x, waves_y = 2 tiles_y
};

// Inclusive ranges of waves, clamped to the frame; nothing when bx0 > bx1 or by0 > by1.
struct CoverageRect { int32_t bx0, bx1, by0, by1; };

RRT_COV_HD inline CoverageRect coverage_whole_frame(const CoverageFrame& F) { return CoverageRect{0, (int32_t)(2u * F.tiles_x) - 1, 0, (int32_t)(2u * F.tiles_y) - 1}; }
RRT_COV_HD inline bool coverage_is_whole_frame(const CoverageFrame& F, const CoverageRect& r) {
    return r.bx0 == 0 && r.by0 == 0 && r.bx1 == (int32_t)(2u * F.tiles_x) - 1 && r.by1 == (int32_t)(2u * F.tiles_y) - 1;
}
// The bit of wave (bx, by) in the mask: render_kernel's block index of a whole frame (tile-major, four quadrants per tile), after its XCD re-labelling.
RRT_COV_HD inline uint32_t coverage_wave_index(uint32_t tiles_x, uint32_t bx, uint32_t by) {
    return (((by >> 1) * tiles_x + (bx >> 1)) << 2) | ((by & 1u) << 1) | (bx & 1u);
}

// The words of a mask: one bit per wave, four per tile, 32 per word (coverage.hip fills them, render_kernel and the getters of frames.cpp read them).
RRT_COV_HD inline uint32_t coverage_words_of(uint32_t tiles_x, uint32_t tiles_y) { return (uint32_t)(((uint64_t)tiles_x * tiles_y + 7u) / 8u); }

// ---- WIDE BOXES AND SIMPLE WAVES (coverage.hip lists them, render_kernel uses them; DESIGN.md section 4, "wide boxes").
// THE RULE.  The rectangle r of list slot `slot` is WIDE when all of these hold:
//   * r holds a wave and is not the whole frame (coverage_is_whole_frame: such a box makes every wave ordinary, as before);
//   * slot < root_end: the slot belongs to the ROOT node's own list, which is the slots [0, root_end) of the built scene (the slots are in node-id order and the
//     root is node 0; the host passes root_end, and 0 -- nothing is wide -- with RRT_FLAG_NO_WIDE_COVER);
//   * r covers at least kWideMinWaves waves AND at least 1 / kWideFrameShare of the frame's waves.
// At most kMaxWide wide boxes are LISTED per frame, whichever the pass comes to first; a wide box that finds the list full is an ordinary box.  Every box that is
// not listed ORs its rectangle into a second mask, `fine`.  A wave whose bit is set in the mask and clear in `fine` is SIMPLE: the only boxes that reach it are
// listed ones.  The bundle-filter render_kernel uses them; the lane-filter and ray-walk kernels are compiled without the path (render.hip: kWidePath) and walk.
// THE THRESHOLD.  A record costs every simple wave one rectangle compare and buys a wave its walk only where NO unlisted box reaches, so the sixteen records
// should go to the boxes that own large parts of the frame.  The share makes that independent of the resolution: the teapot frame has 14 root-list boxes (table
// and mirror) that cover more than 1/81 of the frame each and none between 1/324 and 1/81, at 256 x 144 as at 3840 x 2160; 1/128 lies between.  An absolute count
// alone does not do: 400 waves lists the 14 at 1920 x 1080, but at 3840 x 2160 27 root-list boxes pass it, the list overflows with teapot triangles and no wave is
// simple (tools/coverage_count.py).  kWideMinWaves is the floor under the share for small frames: a record that could spare fewer than sixteen waves their walk
// is not worth a compare in all the others.
// EXACTNESS.  The soundness above says: a (primary ray, triangle) pair the reference accepts has the ray's sub-sample inside the rectangle of the triangle's slot.
// For a simple wave every accepted pair therefore names a LISTED triangle of the root's own list whose rectangle contains the wave.  At the root, entered with
// max_t = +inf for a primary ray, the reference (ray.rs:104-168) keeps the own list's smallest t, the first list position winning a tie, and then asks its
// children; no accepted pair lies below the root, so every child returns None and the walk returns the own-list result.  render_kernel computes exactly that
// for a simple wave: Moller-Trumbore on the listed triangles whose rectangle contains the wave, keeping (t, position) by  t < own_t || (t == own_t && pos < own_pos)
// from own_t = +inf -- a minimum over a set, so the order of the records does not matter.  Whatever turns the mask off (frames.cpp: coverage_state --
// suspects, no cull, eye range, bad basis, small frames; rank tiles, regions and progressive frames have no mask at all) turns this off with it.
constexpr uint32_t kMaxWide = 16, kWideMinWaves = 16, kWideFrameShare = 128;
// One listed box: its slot (the index of its DevTriGeom record) and its rectangle.
struct WideRecord { uint32_t slot; int32_t bx0, bx1, by0, by1; };
// Behind the mask's words and its `whole` word, in the same buffer: the mask `fine` (n_words words), the number of wide boxes that asked for a record (it can
// exceed kMaxWide: min(count, kMaxWide) records are valid), and the records.  Word offsets from the start of the buffer.
RRT_COV_HD inline uint64_t coverage_fine_offset(uint32_t n_words) { return (uint64_t)n_words + 1u; }
RRT_COV_HD inline uint64_t coverage_wide_count_offset(uint32_t n_words) { return 2ull * n_words + 1u; }
RRT_COV_HD inline uint64_t coverage_wide_records_offset(uint32_t n_words) { return 2ull * n_words + 2u; }
RRT_COV_HD inline uint64_t coverage_buffer_words(uint32_t n_words) { return 2ull * n_words + 2u + kMaxWide * (sizeof(WideRecord) / sizeof(uint32_t)); }
// Waves of a rectangle (0 for an empty one).
RRT_COV_HD inline uint64_t coverage_rect_waves(const CoverageRect& r) {
    return r.bx0 <= r.bx1 && r.by0 <= r.by1 ? (uint64_t)(r.bx1 - r.bx0 + 1) * (uint64_t)(r.by1 - r.by0 + 1) : 0ull;
}
// Whether the rectangle r of list slot `slot` is wide (the rule above, without the list's capacity).
RRT_COV_HD inline bool coverage_is_wide(const CoverageFrame& F, const CoverageRect& r, uint32_t slot, uint32_t root_end) {
    const uint64_t waves = coverage_rect_waves(r), frame_waves = 4ull * F.tiles_x * F.tiles_y;
    return slot < root_end && waves >= kWideMinWaves && waves * kWideFrameShare >= frame_waves && !coverage_is_whole_frame(F, r);
}
RRT_COV_HD inline bool coverage_rect_contains(const WideRecord& w, int32_t bx, int32_t by) { return bx >= w.bx0 && bx <= w.bx1 && by >= w.by0 && by <= w.by1; }

// x clamped to [lo, hi] and converted; x is finite
RRT_COV_HD inline int32_t coverage_clamp_i32(double x, double lo, double hi) { return (int32_t)(x < lo ? lo : x > hi ? hi : x); }

// The waves a box in device form (centre c, half-extent h: device_scene.hpp, DevClusterBox) can reach.  The empty box (h < 0) reaches none, a box that is
// unbounded along an axis (h >= FLT_MAX) every one.
RRT_COV_HD inline CoverageRect coverage_rect(const CoverageFrame& F, const float c[3], const float h[3]) {
    if (h[0] < 0.0f || h[1] < 0.0f || h[2] < 0.0f) return CoverageRect{0, -1, 0, -1};
    double xlo = HUGE_VAL, xhi = -HUGE_VAL, ylo = HUGE_VAL, yhi = -HUGE_VAL;
    bool whole = h[0] >= FLT_MAX || h[1] >= FLT_MAX || h[2] >= FLT_MAX;        // unbounded along an axis (the corners below are then of no account)
    for (int k = 0; k < 8; k++) {
        double d[3], ad[3];
        for (int j = 0; j < 3; j++) {
            d[j] = ((double)c[j] + ((k >> j) & 1 ? (double)h[j] : -(double)h[j])) - F.eye[j];
            ad[j] = fabs(d[j]);
        }
        const double a = (F.inv[0][0] * d[0] + F.inv[0][1] * d[1]) + F.inv[0][2] * d[2];
        const double b = (F.inv[1][0] * d[0] + F.inv[1][1] * d[1]) + F.inv[1][2] * d[2];
        const double g = (F.inv[2][0] * d[0] + F.inv[2][1] * d[1]) + F.inv[2][2] * d[2];
        double s = 0.0;
        for (int i = 0; i < 3; i++) s += (fabs(F.inv[i][0]) * ad[0] + fabs(F.inv[i][1]) * ad[1]) + fabs(F.inv[i][2]) * ad[2];
        const double E = kCoverCoordRel * s, g_lo = g - E;
        if (!(g_lo > 0.0)) { whole = true; continue; }       // behind the eye, in its plane, or not a number
        const double rg = 1.0 / g, rg_lo = 1.0 / g_lo;                     // (two divisions per corner: the quotients below are products with these)
        const double qa = a * rg, qb = b * rg;
        const double xd = qa * F.kx, yd = qb * F.ky;
        const double mx = RRT_COVERAGE_MARGIN_SIGN * (kCoverAbsPix + kCoverRelPix * fabs(xd) + 2.0 * fabs(F.kx) * ((fabs(qa) * E + E) * rg_lo));
        const double my = RRT_COVERAGE_MARGIN_SIGN * (kCoverAbsPix + kCoverRelPix * fabs(yd) + 2.0 * fabs(F.ky) * ((fabs(qb) * E + E) * rg_lo));
        xlo = fmin(xlo, xd - mx); xhi = fmax(xhi, xd + mx);
        ylo = fmin(ylo, yd - my); yhi = fmax(yhi, yd + my);
        if (!(xd - mx > -HUGE_VAL && xd + mx < HUGE_VAL && yd - my > -HUGE_VAL && yd + my < HUGE_VAL)) whole = true;   // overflow, or not a number
    }
    if (whole) return coverage_whole_frame(F);
    // wave bx meets [xlo, xhi]  <=>  4 bx - W/2 <= xhi  and  4 bx + 3.5 - W/2 >= xlo;  wave by meets [ylo, yhi]  <=>  top - 4 by - 3 <= yhi  and  top - 4 by + 0.5 >= ylo
    const double wx = 2.0 * (double)F.tiles_x, wy = 2.0 * (double)F.tiles_y;
    CoverageRect r;
    r.bx0 = coverage_clamp_i32(ceil((xlo + F.half_w - 3.5) * 0.25), 0.0, wx);
    r.bx1 = coverage_clamp_i32(floor((xhi + F.half_w) * 0.25), -1.0, wx - 1.0);
    r.by0 = coverage_clamp_i32(ceil((F.top - 3.0 - yhi) * 0.25), 0.0, wy);
    r.by1 = coverage_clamp_i32(floor((F.top + 0.5 - ylo) * 0.25), -1.0, wy - 1.0);
    return r;
}

// The frame's part of the rule from what a launch knows (host).  False: the mask must be off for this frame -- a value that is not finite, z_value <= 0,
// or a basis whose inverse is not good enough for (a) above.
inline bool coverage_frame(CoverageFrame& F, uint32_t width, uint32_t height, double x_scale, double y_scale, double z_value,
                           const double right[3], const double up[3], const double forward[3], const double eye[3]) {
    const double M[3][3] = {{right[0], up[0], forward[0]}, {right[1], up[1], forward[1]}, {right[2], up[2], forward[2]}};
    const double det = M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) + M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
    if (!(fabs(det) > 0.0) || !std::isfinite(det)) return false;
    const double adj[3][3] = {
        {M[1][1] * M[2][2] - M[1][2] * M[2][1], M[0][2] * M[2][1] - M[0][1] * M[2][2], M[0][1] * M[1][2] - M[0][2] * M[1][1]},
        {M[1][2] * M[2][0] - M[1][0] * M[2][2], M[0][0] * M[2][2] - M[0][2] * M[2][0], M[0][2] * M[1][0] - M[0][0] * M[1][2]},
        {M[1][0] * M[2][1] - M[1][1] * M[2][0], M[0][1] * M[2][0] - M[0][0] * M[2][1], M[0][0] * M[1][1] - M[0][1] * M[1][0]}};
    double norm_m = 0.0, norm_i = 0.0, residual = 0.0;
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) F.inv[i][j] = adj[i][j] / det;
    for (int i = 0; i < 3; i++) {
        norm_m = fmax(norm_m, fabs(M[i][0]) + fabs(M[i][1]) + fabs(M[i][2]));
        norm_i = fmax(norm_i, fabs(F.inv[i][0]) + fabs(F.inv[i][1]) + fabs(F.inv[i][2]));
        for (int j = 0; j < 3; j++) {
            const double p = (F.inv[i][0] * M[0][j] + F.inv[i][1] * M[1][j]) + F.inv[i][2] * M[2][j];
            residual = fmax(residual, fabs(p - (i == j ? 1.0 : 0.0)));
        }
    }
    if (!(residual <= kCoverMaxResidual) || !(norm_m * norm_i <= kCoverMaxCond)) return false;     // (false for a NaN too)
    F.kx = z_value / x_scale; F.ky = z_value / y_scale;
    if (!(z_value > 0.0) || !std::isfinite(F.kx) || !std::isfinite(F.ky)) return false;
    for (int j = 0; j < 3; j++) { F.eye[j] = eye[j]; if (!std::isfinite(eye[j])) return false; }
    F.half_w = (double)(width / 2u); F.top = (double)(height - height / 2u);
    F.tiles_x = (width + 7u) / 8u; F.tiles_y = (height + 7u) / 8u;
    return true;
}

}  // namespace rrt
