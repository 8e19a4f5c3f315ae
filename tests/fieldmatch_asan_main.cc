// tests/fieldmatch_asan_main.cc — TEST HARNESS, NOT PRODUCT.  A stand-alone program over tests/emu/fieldmatch.cpp for an AddressSanitizer / UBSan build
// (tests/test_fieldmatch_cpu.py compiles the two files with -fsanitize=address,undefined and runs the result): the stepped k_fm_metrics, k_fm_fold and k_fm_weave
// over source planes that end with the last sample of their last row, every size of the tests, the smallest picture and one with a single column pair past a
// tile, both element types, every alignment class, both keeps.  A read past a source plane, a write past an output plane, the partials or the LDS image, or a
// signed overflow ends the program with the sanitizer's report; exit status 0 otherwise.
#include <cstdint>
#include <cstdio>
#include <vector>

extern "C" int emu_fm_metrics(const void *prev, const void *cur, const void *next, int w, int h, int depth, int keep, int order, int align, unsigned lds_seed,
                              unsigned long long *out, int *stats);
extern "C" int emu_fm_weave(const void *const *cur, const void *const *other, int w, int h, int depth, int keep, int order, int align, void *out_y, void *out_u,
                            void *out_v, int *stats);

int main()
{
    const int sizes[][2] = {{70, 36}, {136, 72}, {264, 20}, {16, 16}, {130, 64}};
    const int aligns[4] = {16, 8, 4, 1};
    uint32_t rnd = 2463534242u;
    int runs = 0;
    for (auto &sz : sizes)
        for (int depth : {8, 10})
            for (int align : aligns)
                for (int keep = 0; keep < 2; keep++) {
                    const int w = sz[0], h = sz[1], es = depth > 8 ? 2 : 1, pw = (w + 7) & ~7, ph = (h + 7) & ~7;
                    std::vector<uint8_t> planes[9];
                    const void *p[3][3];
                    for (int f = 0; f < 3; f++)
                        for (int c = 0; c < 3; c++) {
                            auto &v = planes[3 * f + c];
                            v.resize((size_t)(c ? w * h / 4 : w * h) * es);
                            for (auto &b : v) { rnd = rnd * 1664525u + 1013904223u; b = (uint8_t)(rnd >> 24); }      // 16-bit elements: values above the depth too
                            p[f][c] = v.data();
                        }
                    unsigned long long out[8];
                    int stats[4] = {0, 0, 0, 0};
                    int rc = emu_fm_metrics(p[0][0], p[1][0], p[2][0], w, h, depth, keep, runs % 3, align, (unsigned)runs, out, stats);
                    if (rc || stats[0] || stats[2] != align) {
                        fprintf(stderr, "metrics %dx%d depth %d align %d keep %d: rc %d, misaligned %d, planes of class %d\n", w, h, depth, align, keep, rc, stats[0], stats[2]);
                        return 1;
                    }
                    std::vector<uint8_t> oy((size_t)pw * ph * es), ou((size_t)pw * ph / 4 * es), ov(ou.size());
                    rc = emu_fm_weave(p[1], p[0], w, h, depth, keep, runs % 3, align, oy.data(), ou.data(), ov.data(), stats);
                    if (rc || stats[0] || stats[1] || stats[2] != align || stats[3] != align) {
                        fprintf(stderr, "weave %dx%d depth %d align %d keep %d: rc %d, misaligned %d, spilled %d, planes of class %d / %d\n", w, h, depth, align, keep, rc,
                                stats[0], stats[1], stats[2], stats[3]);
                        return 1;
                    }
                    runs++;
                }
    printf("%d runs\n", runs);
    return 0;
}
