// specular_skip.hpp -- when does the f64 sum  I = I + specular  return I bit for bit?  (render.hip: specular_term)
//
// The reference adds, per light and channel c (raytracer.rs:219-226, 245-252, 279-304),
//     s_c = fl(fl(ks_c * intensity) * P),   P = powf(q_ref, sw),   q_ref = fl(r.v / fl(|r| * |v|)),   |r| = fl(sqrt(fl(r.r))), |v| likewise,
// to the running sum I_c, whenever sw != -1 and r.v > 0.  For most hits P is so small that the addition rounds back to I_c: the term then costs a
// sqrt, a divide and a pow in f64 for nothing.  The functions below decide "certainly absorbed" from fp32 estimates alone.  They are plain
// arithmetic, the same text for host and device (the device takes v_log_f32 and v_rcp_f32 for log2f and 1/x), so that a stand-alone host program
// can check them against the reference's expression (tests/test_specular_skip_model.py).  A "no" is always safe: the caller then evaluates the term.
//
// CLAIM.  Let E2 = spec_log2_pow_x2(rv, rr, vv, sw) with
//     rv = RN32(r.v);   rr, vv = r.r, v.v to within a factor (1 +- 2^-20);   sw = RN32(sw),
// and let |ks_c * intensity| < 2^kexp <= 2^1023 (exact product) and I_c >= 2^iexp be positive, finite and normal.  If spec_absorbed_exp(E2, kexp, iexp)
// holds, then  I_c + s_c == I_c  in round-to-nearest-even f64, for the s_c the reference computes and for every pow within 8 ulps of the true power.
//
// PROOF.
//  (A) Absorption.  Let I > 0 be finite and normal and |s| <= I * 2^-55.  With 2^e <= I < 2^(e+1), the f64 neighbours of I are I + 2^(e-52) above and,
//      below, I - 2^(e-52), or I - 2^(e-53) when I == 2^e (the spacing halves below a power of two; a negative intensity makes s negative, which
//      is why the bound is 2^-55 and not 2^-54).  |s| <= I * 2^-55 < 2^(e-54) is less than half of either gap, so I + s rounds to I.
//  (B) Ranges.  spec_log2_pow_x2 answers +inf ("no") unless rv >= 2^-50, rr >= 2^-60, vv >= 2^-60, rr * vv <= 2^120 and sw >= 2^-126, every
//      comparison false for a NaN.  So r.v > 0 is certain (rv is RN32 of it, and the caller's own test r.v > 0 stays the f64 one), sw > 0
//      (sw <= 0, sw == -1, NaN: "no"; sw = +inf is let through: the power of a q < 1 is then 0, and E2 = -inf says so), all of r.v, r.r, v.v lie in
//      [2^-61, 2^121], and none of the f64 or fp32 operations that form q_ref or the estimate overflows; fp32 underflow is dealt with in (D).
//  (C) q_ref against q = r.v / sqrt(r.r * v.v) (exact quotient of the exact sums of the f64 components' squares).  The reference's r.r is a sum of
//      three non-negative rounded products, relative error <= 3 * 2^-53 and then some; sqrt halves it and rounds; the product of the lengths and the
//      quotient round once each.  In all q_ref = q * (1 + d), |d| < 2^-49 -- slack (i).
//  (D) The estimate Q = fma(rv^2 * rcp(rr * vv), 1 + 2^-12, 2^-120) is an upper bound of q_ref^2.  Relative errors: rv, squared and rounded, 3 * 2^-24;
//      rr and vv, 2^-20 each by contract (spec_sumsq_f32 and spec_sq_f32 below meet it: three conversions, three products, two sums of non-negative
//      terms give (1 +- 2^-24)^5; a term that underflows loses at most 2^-126 in absolute terms against a sum >= 2^-60); their product 2^-24; the
//      reciprocal 2^-23 (v_rcp_f32: 1 ulp; the host divides); the last product 2^-24.  Together below 2^-18 -- slack (ii).  With (i) that uses
//      6e-6 of the 3.5e-4 that the factor 1 + 2^-12 adds to log2 Q; the rest is spent in (F).  The last product may underflow (q^2 can be as small as
//      2^-240): it then loses at most 2^-126 absolutely, flushed or not, which the added 2^-120 covers -- it also keeps Q normal, so that the
//      logarithm below is finite, -120 at the least.  An overflowing rv^2 gives Q = inf: "no".
//  (E) "No" unless Q <= 1 - 2^-10: then 0 < q_ref < 1 certainly, and log2 Q <= -1.4e-3 is a negative number well away from zero, at which one ulp is
//      a relative error of 2^-23.  L = log2(Q) as the hardware (v_log_f32, documented to 1 ulp) or log2f (glibc, < 1 ulp) returns it is allowed
//      FOUR ulps: |L - log2 Q| <= 2^-21 |log2 Q| -- slack (iii).
//  (F) E2 = fl(sw * L) is an upper bound of  2 log2(true power) = sw_f64 * log2 q_ref^2  (both negative).  RN32(sw) is off by 2^-24, L by 2^-21, the product
//      by 2^-24: E2 = sw_f64 * log2 Q * (1 + t), |t| < 2^-20, and |log2 Q| <= 120 makes that at most 1.2e-4 * sw_f64 in absolute terms, while (D) left
//      sw_f64 * (log2 Q - log2 q_ref^2) >= 3.4e-4 * sw_f64.  So a large sw can only push E2 further down, where the true power is smaller still.  A product
//      that underflows moves towards zero (safe); one that overflows gives -inf, where the true exponent is below -2^126.
//  (G) The computed pow.  P <= 2^(E2/2) * (1 + 2^-50) + 2^-1072: a pow within 8 ulps of the true power (OCML and glibc both claim 1 ulp; the model
//      test moves glibc's result by +-2 ulps) -- slack (iv) -- or, where the power is subnormal or underflows, at most a few units of 2^-1074.
//  (H) The comparison, in integers.  fl(ks_c * intensity) is finite and at most 2^kexp in magnitude (2^kexp is a power of two within range, or below half
//      the smallest subnormal, where the product rounds to 0).  The test  max(E2, -2144) <= 2 (iexp - kexp - 57)  gives, first, kexp - iexp <= 1015, and
//          |s_c| <= 2^kexp * P * (1 + 2^-53) + 2^-1075 <= 2^kexp * 2^(iexp - kexp - 57) * (1 + 2^-49) + 2^(kexp - 1072) + 2^-1075 < 2^iexp * 2^-55 <= I_c * 2^-55,
//      with a factor of two to spare; (A) finishes.  Integer arithmetic on the exponents is exact, and so is the conversion of the right side to fp32.
//      spec_absorbed3 takes kexp and iexp from the exponent FIELDS of the f64 operands: |x| < 2^(field - 1022) for every finite x, subnormals and zero
//      included; a field of 0x7FF (inf, NaN) is a "no".  The three sums are taken by their high words as signed integers: the smallest must be at least
//      0x00100000 (positive and normal: no zero, no subnormal, no negative number), the largest below 0x7FF00000 (no inf, no NaN); of positive numbers
//      the smallest high word belongs to the smallest number's binade.  One kexp (the largest |ks_c|) and one iexp (the smallest I_c) serve all channels.
//  (I) A channel with ks_c == 0 adds +-0 * P, and P is finite by (E): any finite I_c other than -0 absorbs it (spec_absorbed, the one-channel form;
//      -0 + +0 is +0).  The kernels do not use this case: a material with a zero ks channel is simply bounded by its largest.
//
// What the slack costs: ns = 240, ks * intensity = 1, I = 0.5 skips below q = 0.843 - 0.003.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define RRT_SPEC_HD __host__ __device__
#else
#define RRT_SPEC_HD
#endif

namespace rrt {

RRT_SPEC_HD inline float spec_log2(float x) {      // x normal, 2^-120 <= x < 1; allowed 4 ulps, (E)
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_logf(x);               // v_log_f32
#else
    return log2f(x);
#endif
}
RRT_SPEC_HD inline float spec_rcp(float x) {       // x normal, 2^-120 <= x <= 2^120; allowed 1 ulp, (D)
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_rcpf(x);               // v_rcp_f32
#else
    return 1.0f / x;
#endif
}
RRT_SPEC_HD inline int spec_hi(double x) { uint64_t b; __builtin_memcpy(&b, &x, 8); return (int)(uint32_t)(b >> 32); }   // the high word, as a signed integer
RRT_SPEC_HD inline int spec_exp_field(double x) { return (spec_hi(x) >> 20) & 0x7FF; }                                      // |x| < 2^(field - 1022) if field < 0x7FF

// x.x of an f64 vector, and the square of an f64 length, in fp32 to within (1 +- 2^-20) -- see (D)
RRT_SPEC_HD inline float spec_sumsq_f32(double x, double y, double z) {
    const float a = (float)x, b = (float)y, c = (float)z;
    return (a * a + b * b) + c * c;
}
RRT_SPEC_HD inline float spec_sq_f32(double len) { const float a = (float)len; return a * a; }

// E2 of (F): twice an upper bound of log2 of the reference's pow(q_ref, sw); +inf where the argument does not apply, (B) and (E).
RRT_SPEC_HD inline float spec_log2_pow_x2(float rv, float rr, float vv, float sw) {
    const float den = rr * vv;
    const float q2 = __builtin_fmaf((rv * rv) * spec_rcp(den), 1.0f + 0x1p-12f, 0x1p-120f);
    const bool applies = rv >= 0x1p-50f && rr >= 0x1p-60f && vv >= 0x1p-60f && den <= 0x1p120f && sw >= 0x1p-126f && q2 <= 1.0f - 0x1p-10f;
    if (!applies) return __builtin_huge_valf();
    return sw * spec_log2(q2);
}
// (H): |ks_c * intensity| < 2^kexp <= 2^1023, I_c >= 2^iexp positive, finite and normal
RRT_SPEC_HD inline bool spec_absorbed_exp(float e2, int kexp, int iexp) {
    return (e2 < -2144.0f ? -2144.0f : e2) <= (float)(2 * (iexp - kexp - 57));
}
RRT_SPEC_HD inline int spec_min3(int a, int b, int c) { const int m = a < b ? a : b; return m < c ? m : c; }
RRT_SPEC_HD inline int spec_max3(int a, int b, int c) { const int m = a > b ? a : b; return m > c ? m : c; }
// All three channels at once, as the kernels ask, straight from the f64 operands' exponent fields -- (H)
RRT_SPEC_HD inline bool spec_absorbed3(float e2, double ks_x, double ks_y, double ks_z, double intensity, double i_x, double i_y, double i_z) {
    const int ea = spec_max3(spec_exp_field(ks_x), spec_exp_field(ks_y), spec_exp_field(ks_z)), eb = spec_exp_field(intensity);
    const int lo = spec_min3(spec_hi(i_x), spec_hi(i_y), spec_hi(i_z)), hi = spec_max3(spec_hi(i_x), spec_hi(i_y), spec_hi(i_z));
    if (!(ea < 0x7FF && eb < 0x7FF && ea + eb <= 2044 + 1023 && lo >= 0x00100000 && hi < 0x7FF00000)) return false;
    return spec_absorbed_exp(e2, ea + eb - 2044, (lo >> 20) - 1023);
}
// One channel from f64 operands: the form the model program sweeps.  ksi = fl(ks_c * intensity).
RRT_SPEC_HD inline bool spec_absorbed(double r_dot_v, double rr, double vv, double sw, double ksi, double i_c) {
    const float e2 = spec_log2_pow_x2((float)r_dot_v, (float)rr, (float)vv, (float)sw);
    if (!(e2 <= 0.0f)) return false;
    const int hi = spec_hi(i_c);
    if (ksi == 0.0) return (hi & 0x7FF00000) != 0x7FF00000 && !(i_c == 0.0 && hi < 0);   // (I)
    if (!(spec_exp_field(ksi) < 0x7FF && hi >= 0x00100000 && hi < 0x7FF00000)) return false;
    return spec_absorbed_exp(e2, spec_exp_field(ksi) - 1022, (hi >> 20) - 1023);
}

}  // namespace rrt
