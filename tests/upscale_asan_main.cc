// tests/upscale_asan_main.cc — TEST HARNESS, NOT PRODUCT.  A stand-alone program over tests/emu/upscale.cpp for an AddressSanitizer / UBSan build
// (tests/test_upscale_cpu.py compiles the two files with -fsanitize=address,undefined and runs the result): the stepped k_upscale and the table builder over
// source planes that end with the last sample of their last row, every ratio of the tests, element type, alignment class and setting, at output sizes with and
// without a margin.  A read past a source plane or a table, a write past an output plane or an LDS image, or a signed overflow ends the program with the
// sanitizer's report; exit status 0 otherwise.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../include/mihevc.h"

extern "C" int emu_upscale(const mihevc_upscale_src *src, const void *y, const void *u, const void *v, int dw, int dh, int out_depth, int order, int align,
                           unsigned lds_seed, void *out_y, void *out_u, void *out_v, int *stats);

int main()
{
    // source size -> output size: 1:1, 3:2, 2:1, 4:1, 2:1 by 1:1, an uneven ratio; then onto a size with a margin; the smallest picture at 1:1 and at 1:4
    const int cases[][4] = {{136, 72, 136, 72}, {90, 48, 136, 72}, {68, 36, 136, 72}, {34, 18, 136, 72}, {68, 72, 136, 72}, {50, 26, 136, 72},
                            {70, 38, 70, 38},   {46, 26, 70, 38},  {36, 20, 70, 38},  {18, 16, 70, 38},  {16, 16, 16, 16},  {16, 16, 64, 64}};
    const int aligns[4] = {16, 8, 4, 1}, depths[3] = {8, 10, 16}, settings[4][2] = {{0, 0}, {0, 8}, {8, 8}, {64, 5}};
    uint32_t rnd = 12345;
    int runs = 0;
    for (auto &cs : cases)
        for (int bits : depths)
            for (int align : aligns)
                for (int out_depth : {8, 10}) {
                    const int *st = settings[runs & 3];
                    const mihevc_upscale_src f = {cs[0], cs[1], bits, st[0], st[1], {0, 0, 0}};
                    const int sw = cs[0], sh = cs[1], dw = cs[2], dh = cs[3], es = bits > 8 ? 2 : 1, pw = (dw + 7) & ~7, ph = (dh + 7) & ~7;
                    std::vector<uint8_t> y((size_t)sw * sh * es), u((size_t)sw * sh / 4 * es), v(u.size());
                    for (auto *p : {&y, &u, &v})
                        for (auto &b : *p) { rnd = rnd * 1664525u + 1013904223u; b = (uint8_t)(rnd >> 24); }      // 16-bit elements: values above the depth too
                    const size_t eo = out_depth > 8 ? 2 : 1;
                    std::vector<uint8_t> oy((size_t)pw * ph * eo), ou((size_t)pw * ph / 4 * eo), ov(ou.size());
                    int stats[4] = {0, 0, 0, 0};
                    const int rc = emu_upscale(&f, y.data(), u.data(), v.data(), dw, dh, out_depth, runs % 3, align, (unsigned)runs, oy.data(), ou.data(), ov.data(), stats);
                    if (rc || stats[0] || stats[1] || stats[2] != align || stats[3] != align) {
                        fprintf(stderr, "%dx%d -> %dx%d bits %d align %d -> %d: rc %d, misaligned %d, spilled %d, planes of class %d / %d\n", sw, sh, dw, dh, bits, align,
                                out_depth, rc, stats[0], stats[1], stats[2], stats[3]);
                        return 1;
                    }
                    runs++;
                }
    printf("%d runs\n", runs);
    return 0;
}
