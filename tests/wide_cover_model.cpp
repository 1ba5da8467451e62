// Stand-alone host check of the wide-box part of csrc/coverage_rule.hpp (tests/test_wide_cover_restatement.py builds and runs it; never linked into the library).
//   wide_cover_model IN OUT     ("-" is stdin / stdout) reads (frame, box, slot, root_end) tuples in binary and writes what the header makes of each, taking the
//   boxes of a frame one after the other as ONE pass over them would: the count of wide boxes starts at 0 where `first` is set and goes up with every wide box, and
//   a wide box is listed while the count it finds is below kMaxWide.
//       in, 168 bytes:  uint32 width, height; double x_scale, y_scale, z_value, right[3], up[3], forward[3], eye[3]; float c[3], h[3]; uint32 slot, root_end, first, pad
//       out, 40 bytes:  int32 ok (coverage_frame), bx0, bx1, by0, by1 (coverage_rect), whole (coverage_is_whole_frame), wide (coverage_is_wide), listed;
//                       uint64 waves (coverage_rect_waves)          (everything after ok is 0 where ok is 0)
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "coverage_rule.hpp"

using namespace rrt;

struct TupleIn { uint32_t width, height; double x_scale, y_scale, z_value, right[3], up[3], forward[3], eye[3]; float c[3], h[3]; uint32_t slot, root_end, first, pad; };
struct TupleOut { int32_t ok, bx0, bx1, by0, by1, whole, wide, listed; uint64_t waves; };
static_assert(sizeof(TupleIn) == 168 && sizeof(TupleOut) == 40, "the record layouts tests/test_wide_cover_restatement.py reads and writes");
static_assert(sizeof(WideRecord) == 20, "the record render_kernel reads: five words");

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: wide_cover_model IN OUT\n"); return 2; }
    FILE* in = strcmp(argv[1], "-") ? fopen(argv[1], "rb") : stdin;
    FILE* out = strcmp(argv[2], "-") ? fopen(argv[2], "wb") : stdout;
    if (!in || !out) { fprintf(stderr, "cannot open %s or %s\n", argv[1], argv[2]); return 2; }
    // the buffer's layout: mask, `whole`, `fine`, the count, sixteen records of five words
    if (coverage_fine_offset(10) != 11 || coverage_wide_count_offset(10) != 21 || coverage_wide_records_offset(10) != 22 || coverage_buffer_words(10) != 22 + 16 * 5) { fprintf(stderr, "buffer layout\n"); return 3; }
    TupleIn p;
    uint32_t count = 0;
    while (fread(&p, sizeof p, 1, in) == 1) {
        TupleOut o;
        memset(&o, 0, sizeof o);
        if (p.first) count = 0;
        CoverageFrame F;
        if (coverage_frame(F, p.width, p.height, p.x_scale, p.y_scale, p.z_value, p.right, p.up, p.forward, p.eye)) {
            const CoverageRect r = coverage_rect(F, p.c, p.h);
            o.ok = 1; o.bx0 = r.bx0; o.bx1 = r.bx1; o.by0 = r.by0; o.by1 = r.by1; o.whole = coverage_is_whole_frame(F, r) ? 1 : 0;
            o.waves = coverage_rect_waves(r);
            o.wide = coverage_is_wide(F, r, p.slot, p.root_end) ? 1 : 0;
            if (o.wide) o.listed = count++ < kMaxWide ? 1 : 0;
        }
        if (fwrite(&o, sizeof o, 1, out) != 1) { fprintf(stderr, "short write\n"); return 2; }
    }
    if (out != stdout) fclose(out); else fflush(out);
    if (in != stdin) fclose(in);
    return 0;
}
