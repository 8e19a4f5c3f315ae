// tests/mcfi_asan_main.cc — TEST HARNESS, NOT PRODUCT.  A stand-alone program over tests/emu/mcfi.cpp for an AddressSanitizer / UBSan build
// (tests/test_mcfi_cpu.py compiles the two files with -fsanitize=address,undefined and runs the result): the stepped k_mcfi_search, k_mcfi_field and k_mcfi_render
// over source planes that end with the last sample of their last row, every size of the tests, both element types, every alignment class; the render with the
// searched field and with the extreme ones (+18 and -18 in every block, signs alternating from block to block).  A read past a source plane, a write past an
// output plane, the device block or the LDS images, or a signed overflow ends the program with the sanitizer's report; exit status 0 otherwise.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../include/mihevc.h"

extern "C" int emu_mcfi_vectors(const void *cur_y, const void *next_y, int w, int h, int depth, int order, int align, unsigned lds_seed, int16_t *v0, int16_t *v,
                                uint64_t *scene_sum, int *stats);
extern "C" int emu_mcfi_render(const mihevc_interpolate *m, int j, const void *const *cur, const void *const *next, const int16_t *v, uint64_t scene_sum, int w, int h,
                               int depth, int order, int align, unsigned lds_seed, void *out_y, void *out_u, void *out_v, int *stats);

int main()
{
    const int sizes[][2] = {{16, 16}, {70, 36}, {72, 72}, {138, 74}};
    const int aligns[4] = {16, 8, 4, 1};
    uint32_t rnd = 2463534242u;
    int runs = 0;
    for (auto &sz : sizes)
        for (int depth : {8, 10})
            for (int align : aligns) {
                const int w = sz[0], h = sz[1], es = depth > 8 ? 2 : 1, pw = (w + 7) & ~7, ph = (h + 7) & ~7, nbx = (w + 7) / 8, nby = (h + 7) / 8;
                std::vector<uint8_t> planes[6];
                const void *p[2][3];
                for (int f = 0; f < 2; f++)
                    for (int c = 0; c < 3; c++) {
                        auto &v = planes[3 * f + c];
                        v.resize((size_t)(c ? w * h / 4 : w * h) * es);
                        for (auto &b : v) { rnd = rnd * 1664525u + 1013904223u; b = (uint8_t)(rnd >> 24); }      // 16-bit elements: values above the depth too
                        p[f][c] = v.data();
                    }
                std::vector<int16_t> field[4];
                for (auto &f : field) f.resize((size_t)nbx * nby * 2);
                uint64_t sum = 0;
                int stats[4] = {0, 0, 0, 0};
                int rc = emu_mcfi_vectors(p[0][0], p[1][0], w, h, depth, runs % 3, align, (unsigned)runs, field[1].data(), field[0].data(), &sum, stats);
                if (rc || stats[0] || stats[2] != align) {
                    fprintf(stderr, "vectors %dx%d depth %d align %d: rc %d, misaligned %d, planes of class %d\n", w, h, depth, align, rc, stats[0], stats[2]);
                    return 1;
                }
                runs++;
                for (int b = 0; b < nbx * nby; b++) {
                    const int16_t alt = (int16_t)(((b % nbx + b / nbx) & 1) ? 18 : -18);
                    field[1][2 * b] = field[1][2 * b + 1] = 18; field[2][2 * b] = field[2][2 * b + 1] = -18; field[3][2 * b] = alt; field[3][2 * b + 1] = (int16_t)-alt;
                }
                for (int k = 0; k < 4; k++) {
                    const mihevc_interpolate m = {2 + k % 3, 0, k ? 0 : 10, {0, 0, 0, 0, 0}};
                    std::vector<uint8_t> oy((size_t)pw * ph * es), ou((size_t)pw * ph / 4 * es), ov(ou.size());
                    rc = emu_mcfi_render(&m, 1, p[0], p[1], field[k].data(), sum, w, h, depth, runs % 3, align, (unsigned)runs, oy.data(), ou.data(), ov.data(), stats);
                    if (rc || stats[0] || stats[1] || stats[2] != align || stats[3] != align) {
                        fprintf(stderr, "render %dx%d depth %d align %d field %d: rc %d, misaligned %d, spilled %d, planes of class %d / %d\n", w, h, depth, align, k, rc,
                                stats[0], stats[1], stats[2], stats[3]);
                        return 1;
                    }
                    runs++;
                }
            }
    printf("%d runs\n", runs);
    return 0;
}
