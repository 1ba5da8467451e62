// Stand-alone model check of csrc/specular_skip.hpp (built and run by tests/test_specular_skip_model.py; never loaded into Python).
//   specular_skip_model N  ->  one line "tuples=... absorbed=... near_threshold=... vector_tuples=... vector_absorbed=... band_share=... failures=..."
// Exit status 0 iff no tuple that the predicate called absorbed changes the sum: for each such tuple the reference's expression
//   s = ksi * pow(r.v / (sqrt(r.r) * sqrt(v.v)), sw)
// is evaluated in f64 with the C library's pow, and with that pow moved by +-1 and +-2 ulps (another library's pow), and I + s must be I bit for bit.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "specular_skip.hpp"

namespace {

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() { uint64_t z = (g_state += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
double uni() { return (double)(rnd() >> 11) * 0x1p-53; }                       // [0, 1)
double uni(double a, double b) { return a + (b - a) * uni(); }
double log_uni(double e0, double e1) { return std::exp2(uni(e0, e1)); }         // 2^[e0, e1)
uint64_t bits(double x) { uint64_t b; std::memcpy(&b, &x, 8); return b; }
double step_ulps(double x, int n) { for (; n > 0; n--) x = std::nextafter(x, HUGE_VAL); for (; n < 0; n++) x = std::nextafter(x, -HUGE_VAL); return x; }

const double kSpecial[] = {0.0, -0.0, HUGE_VAL, -HUGE_VAL, NAN, -NAN, 4.9406564584124654e-324, -4.9406564584124654e-324, 1e-310, DBL_MIN, -DBL_MIN, DBL_MAX, -DBL_MAX, 1.0, -1.0,
                           0x1p-126, 0x1p-127, 0x1p-149, 0x1p-150, 0x1p127, 0x1p128, 0x1p-60, 0x1p-61, 0x1p60, 0x1p120};
double special() { return kSpecial[rnd() % (sizeof kSpecial / sizeof kSpecial[0])]; }

unsigned long long g_failures = 0;
// the reference's addition for one channel; true iff I + s == I for the library's pow and its neighbours
bool sum_unchanged(double rv, double rr, double vv, double sw, double ksi, double i_c) {
    const double q = rv / (std::sqrt(rr) * std::sqrt(vv));
    const double p = std::pow(q, sw);
    for (int d = -2; d <= 2; d++) {
        const double s = ksi * step_ulps(p, d);
        if (bits(i_c + s) != bits(i_c)) return false;
    }
    return true;
}
void report(const char* what, double rv, double rr, double vv, double sw, double ksi, double i_c) {
    if (g_failures++ < 10) std::printf("FAIL %s: r.v=%a r.r=%a v.v=%a sw=%a ksi=%a I=%a\n", what, rv, rr, vv, sw, ksi, i_c);
}

double draw_sw() {
    switch (rnd() % 8) {
        case 0: { const double t[] = {0.5, 1.0, 2.0, 10.0, 240.0, 500.0, 1e4, 1e6}; return t[rnd() % 8]; }
        case 1: { const double t[] = {-1.0, 0.0, -0.0, -3.0, -240.0}; return (rnd() & 1) ? t[rnd() % 5] : -log_uni(-10, 40); }
        default: return log_uni(-10, 40);
    }
}
double draw_i() {
    switch (rnd() % 4) {
        case 0: return uni(0.05, 2.0);
        case 1: return log_uni(-1080, 100);                                     // subnormal ... 2^100
        case 2: return log_uni(-140, 20);                                       // around the fp32 normal limit
        default: return (rnd() % 16 == 0 ? -1.0 : 1.0) * log_uni(-40, 10);
    }
}
double draw_ksi() {
    const double sign = (rnd() & 1) ? -1.0 : 1.0;                               // both signs of intensity
    switch (rnd() % 4) {
        case 0: return sign * log_uni(-1074, 1023);
        case 1: return sign * uni();
        default: return sign * log_uni(-30, 70);
    }
}

}  // namespace

int main(int argc, char** argv) {
    const unsigned long long n = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 10000000ull;
    unsigned long long tuples = 0, absorbed = 0, near_thr = 0;
    // ---- one channel from f64 operands
    while (tuples < n) {
        double rr = log_uni(-70, 70), vv = log_uni(-70, 70), sw = draw_sw(), ksi = draw_ksi(), i_c = draw_i();
        if (rnd() % 32 == 0) { rr = log_uni(-130, 130); vv = log_uni(-130, 130); }
        const double scale = std::sqrt(rr) * std::sqrt(vv);
        double q = (rnd() % 8 == 0) ? uni(0.9, 1.1) : uni();
        if (rnd() % 64 == 0) q = -q;
        double rv = q * scale;
        // zeros, infinities, NaNs, subnormals and range limits in every slot
        const uint64_t sp = rnd();
        if ((sp & 0xF) == 0) rv = special();
        if ((sp & 0xF0) == 0) rr = special();
        if ((sp & 0xF00) == 0) vv = special();
        if ((sp & 0xF000) == 0) sw = special();
        if ((sp & 0xF0000) == 0) ksi = special();
        if ((sp & 0xF00000) == 0) i_c = special();
        tuples++;
        if (rrt::spec_absorbed(rv, rr, vv, sw, ksi, i_c)) { absorbed++; if (!sum_unchanged(rv, rr, vv, sw, ksi, i_c)) report("sweep", rv, rr, vv, sw, ksi, i_c); }
        // q on both sides of this tuple's threshold and within a few fp32 ulps of it: bisect r.v for where the predicate flips
        if ((sp >> 60) < 4 && scale > 0.0 && scale < HUGE_VAL) {
            double lo = 0.0, hi = scale;                                        // q = 0 ... 1
            if (rrt::spec_absorbed(0x1p-40 * scale, rr, vv, sw, ksi, i_c) && !rrt::spec_absorbed(hi, rr, vv, sw, ksi, i_c)) {
                lo = 0x1p-40 * scale;
                for (int it = 0; it < 40; it++) { const double mid = 0.5 * (lo + hi); (rrt::spec_absorbed(mid, rr, vv, sw, ksi, i_c) ? lo : hi) = mid; }
                for (int j = -6; j <= 6 && tuples < n; j++) {
                    const double t = lo * (1.0 + j * 0x1p-24);
                    tuples++; near_thr++;
                    if (rrt::spec_absorbed(t, rr, vv, sw, ksi, i_c)) { absorbed++; if (!sum_unchanged(t, rr, vv, sw, ksi, i_c)) report("threshold", t, rr, vv, sw, ksi, i_c); }
                }
            }
        }
    }
    // ---- three channels from vectors, with the arithmetic of render.hip's specular_term: one exponent for ks * intensity, one for the smallest of the three sums
    unsigned long long vec_tuples = 0, vec_absorbed = 0;
    for (; vec_tuples < n / 4; vec_tuples++) {
        double r[3], v[3], ks[3], I[3];
        const double rs = log_uni(-40, 40), vs = log_uni(-40, 40);
        for (int c = 0; c < 3; c++) { r[c] = rs * uni(-1, 1) * (rnd() % 8 ? 1.0 : log_uni(-200, 0)); v[c] = vs * uni(-1, 1); }
        const double kscale = (rnd() & 1) ? 1.0 : log_uni(-400, 60);
        for (int c = 0; c < 3; c++) { ks[c] = kscale * ((rnd() % 4) ? uni() : (rnd() % 2 ? 0.0 : log_uni(-320, 0))); }
        const double i0 = draw_i();
        for (int c = 0; c < 3; c++) I[c] = (rnd() % 4) ? i0 * uni(0.5, 2.0) : draw_i();
        double intensity = ((rnd() & 1) ? -1.0 : 1.0) * ((rnd() & 1) ? uni(0.1, 2.0) : log_uni(-100, 400)), sw = draw_sw();
        const uint64_t sp = rnd();
        if ((sp & 0x1F) == 0) r[rnd() % 3] = special();
        if ((sp & 0x3E0) == 0) v[rnd() % 3] = special();
        if ((sp & 0x7C00) == 0) ks[rnd() % 3] = special();
        if ((sp & 0xF8000) == 0) I[rnd() % 3] = special();
        if ((sp & 0x1F00000) == 0) intensity = special();
        const double rv = (r[0] * v[0] + r[1] * v[1]) + r[2] * v[2];
        if (!(rv > 0.0)) continue;                                              // the kernel's own f64 decision
        const double rr = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2], vv = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2], len_v = std::sqrt(vv);
        const float e2 = rrt::spec_log2_pow_x2((float)rv, rrt::spec_sumsq_f32(r[0], r[1], r[2]), rrt::spec_sq_f32(len_v), (float)sw);
        if (!rrt::spec_absorbed3(e2, ks[0], ks[1], ks[2], intensity, I[0], I[1], I[2])) continue;
        vec_absorbed++;
        for (int c = 0; c < 3; c++) if (!sum_unchanged(rv, rr, vv, sw, ks[c] * intensity, I[c])) report("vector", rv, rr, vv, sw, ks[c] * intensity, I[c]);
    }
    // ---- the teapot-like band: ns = 240, I in [0.05, 2], |ks * intensity| <= 1, q uniform in (0, 1)
    unsigned long long band = 0, band_skipped = 0;
    for (; band < 1000000ull; band++) {
        const double rr = uni(0.5, 4.0), vv = uni(0.5, 4.0), q = uni(), ksi = uni(-1, 1), i_c = uni(0.05, 2.0);
        const double rv = q * std::sqrt(rr) * std::sqrt(vv);
        if (rrt::spec_absorbed(rv, rr, vv, 240.0, ksi, i_c)) { band_skipped++; if (!sum_unchanged(rv, rr, vv, 240.0, ksi, i_c)) report("band", rv, rr, vv, 240.0, ksi, i_c); }
    }
    std::printf("tuples=%llu absorbed=%llu near_threshold=%llu vector_tuples=%llu vector_absorbed=%llu band_share=%.4f failures=%llu\n", tuples, absorbed, near_thr, vec_tuples,
                vec_absorbed, (double)band_skipped / (double)band, g_failures);
    return g_failures ? 1 : 0;
}
