// tests/sr_yuv_asan_main.cc — TEST HARNESS, NOT PRODUCT.  A stand-alone program over tests/emu/sr_yuv.cpp for an AddressSanitizer / UBSan build
// (tests/test_sr_yuv_cpu.py compiles the two files with -fsanitize=address,undefined and runs the result): the stepped k_sr_from_yuv over source planes that
// hold exactly (pitch (rows - 1) + row) elements, the most the definition lets the kernel touch, and a tensor of exactly its size; every depth, matrix, range
// and scale, sizes from 4x4 to more than two workgroups, tight and loose pitches, planes on and one element off an aligned address; then one whole network of
// each scale over an arena of exactly the stated size.  A read or write past a plane, the tensor or the arena, or a signed overflow, ends the program with the
// sanitizer's report.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../include/mihevc.h"

extern "C" int emu_sr_from_yuv(const mihevc_sr_yuv *src, int scale, const void *y, const void *u, const void *v, int pitch_y, int pitch_c, uint16_t *out,
                               int off_one, int order);
extern "C" int emu_sr_network_yuv(const mihevc_sr_model *model, const float *weights, size_t count, const mihevc_sr_yuv *src, const void *y, const void *u,
                                  const void *v, int pitch_y, int pitch_c, uint16_t *out, int order, unsigned lds_seed);

// the flat weight count of an RRDBNet (csrc/sr_net.h): 3x3 kernels and biases of conv_first, `blocks` x 3 x 5 dense layers, conv_body, two up layers, hr, last
static size_t weight_count(int scale, int blocks)
{
    auto layer = [](size_t cin, size_t cout) { return cout * cin * 9 + cout; };
    size_t n = layer(scale == 2 ? 12 : 3, 64);
    for (int k = 0; k < 4; k++) n += (size_t)blocks * 3 * layer(64 + 32 * k, 32);
    n += (size_t)blocks * 3 * layer(192, 64);
    return n + 4 * layer(64, 64) + layer(64, 3);
}

int main()
{
    uint32_t rnd = 4321;
    auto next = [&]() { rnd = rnd * 1664525u + 1013904223u; return rnd >> 8; };
    const int sizes[][2] = {{4, 4}, {18, 14}, {34, 16}, {66, 34}, {6, 260}};
    int runs = 0;
    for (int depth : {8, 10, 12})
        for (int matrix : {1, 5, 6, 9})
            for (int full : {0, 1})
                for (int scale : {4, 2})
                    for (auto &sz : sizes) {
                        const int w = sz[0], h = sz[1], es = depth > 8 ? 2 : 1, py = w + (runs % 3), pc = w / 2 + (runs % 4), off_one = runs & 1;
                        const mihevc_sr_yuv src = {w, h, depth, matrix, full, {0, 0, 0}};
                        std::vector<uint8_t> p[3];
                        for (int c = 0; c < 3; c++) {
                            const int row = c ? w / 2 : w, rows = c ? h / 2 : h, pitch = c ? pc : py;
                            p[c].resize(((size_t)pitch * (rows - 1) + row) * es);
                            for (auto &b : p[c]) b = (uint8_t)next();      // (16-bit samples above the depth included)
                        }
                        std::vector<uint16_t> out((size_t)w * h * 32 / (scale == 2 ? 4 : 1));
                        const int rc = emu_sr_from_yuv(&src, scale, p[0].data(), p[1].data(), p[2].data(), py, pc, out.data(), off_one, runs % 3);
                        if (rc) { fprintf(stderr, "from_yuv depth %d matrix %d full %d scale %d %dx%d: rc %d\n", depth, matrix, full, scale, w, h, rc); return 1; }
                        runs++;
                    }
    for (int scale : {4, 2}) {
        const size_t count = weight_count(scale, 1);
        std::vector<float> w(count);
        for (auto &v : w) v = ((float)(int)(next() % 2001) - 1000.0f) * 2e-5f;
        const mihevc_sr_yuv src = {6, 10, 8, 6, 0, {0, 0, 0}};
        std::vector<uint8_t> y(60), u(15), v(15);
        for (auto *t : {&y, &u, &v}) for (auto &b : *t) b = (uint8_t)next();
        std::vector<uint16_t> out((size_t)3 * 60 * scale * scale);
        const mihevc_sr_model m = {scale, 1, {0, 0, 0, 0, 0, 0}};
        const int rc = emu_sr_network_yuv(&m, w.data(), count, &src, y.data(), u.data(), v.data(), 6, 3, out.data(), 2, 99u);
        if (rc) { fprintf(stderr, "network x%d: rc %d\n", scale, rc); return 1; }
        runs++;
    }
    printf("%d runs\n", runs);
    return 0;
}
