// tests/emu/lut3d.cpp — TEST HARNESS, NOT PRODUCT (part of tests/emu/libkernel_emu.so).  The colour table program of hevc_amd/csrc/kernels/lut3d.h (k_lut3d) stepped on
// the CPU with the sequential executor, every workgroup of the launch.  Source planes and output planes are those of the stepped converters (ingest_planes.h): the
// three source planes allocated to their exact size with the alignment the case asks for, the packed table allocated to its exact size too (a read past either is a
// finding of the AddressSanitizer program tests/test_lut3d_cpu.py builds from this file and tests/lut3d_asan_main.cc), outputs garbage-filled.  The kernel has no
// LDS.  hevc_amd/ never loads this library.
#include <memory>

#include "ingest_planes.h"
#include "../../hevc_amd/csrc/kernels/lut3d.h"

using namespace mihevc;

namespace {

template <typename TI, typename TO>
int run(const mihevc_lut3d_src &f, int n, const uint16_t *table, const void *const *src, int w, int h, int out_depth, int out_matrix, int out_full, int order, int align,
        void *const *out, int *stats)
{
    const int pw = (w + 7) & ~7, ph = (h + 7) & ~7;
    IngestSrcPlane<TI> sp[3];
    for (int c = 0; c < 3; c++)
        if (!sp[c].place(src[c], c ? w / 2 : w, c ? h / 2 : h, align)) return -5;
    const size_t entries = (size_t)n * n * n;
    void *packed = nullptr;
    if (posix_memalign(&packed, 64, entries * LUT_ENTRY_BYTES)) return -5;
    std::unique_ptr<void, decltype(&free)> hold(packed, &free);
    lut3d_pack(n, table, (uint16_t *)packed);
    IngestOutPlanes<TO> op(pw, ph);
    const Lut3dArgs a = lut3d_args(f, n, packed, sp[0].p, sp[1].p, sp[2].p, sp[0].pitch, sp[1].pitch, w, h, pw, ph, out_depth, out_matrix, out_full != 0, op.dst, op.stride);
    stats[2] = a.align[0]; stats[3] = a.align[1];
    SeqExec ex;
    ex.order = order;
    g_ingest_misaligned = 0;
    const int nwg = ingest_rgb_workgroups(pw, ph);
    for (int wg = 0; wg <= nwg; wg++) lut3d_tile_program<TI, TO>(ex, a, wg);     // one past the last: writes nothing
    stats[0] = g_ingest_misaligned;
    stats[1] = op.copy_back(out);
    return 0;
}

}  // namespace

extern "C" {

// the workgroup's tile in source pixels
void emu_lut3d_tile(int *tw, int *th) { *tw = RGB_TW; *th = RGB_TH; }

// the five integer coefficients of step 2 as the host builder makes them: nY, nRv, nGu, nGv, nBu.  Returns 0, or -3 for an unknown matrix
int emu_lut3d_inverse(int matrix, int full, int bits, int *c)
{
    int cc[5];
    if (!lut3d_inverse(matrix, full != 0, bits, cc)) return -3;
    for (int i = 0; i < 5; i++) c[i] = cc[i];
    return 0;
}

// the kernel's division by 65535 (lut_div65535) against the language's at every place where the quotient steps and at the ends of the range: for every
// q = 0 .. 65535 the dividends 65535 q - 1, 65535 q, 65535 q + 1 and 65535 q + 65534 (the form is non-decreasing in x, so agreement at the first and the last
// dividend of every quotient is agreement everywhere), the largest dividend of the blend 65535^2 + 32767, and all of 0 .. 65535 * 64, the range of p.
// Returns the number of wrong quotients
int emu_lut3d_div_check()
{
    int bad = 0;
    for (uint64_t q = 0; q <= 65535; q++)
        for (uint64_t x : {65535 * q - 1, 65535 * q, 65535 * q + 1, 65535 * q + 65534})
            if (x < 65535ull * 65536ull) bad += lut_div65535((uint32_t)x) != (uint32_t)(x / 65535);
    bad += lut_div65535(65535u * 65535u + 32767u) != (65535u * 65535u + 32767u) / 65535u;
    for (uint32_t x = 0; x <= 65535u * 64u; x++) bad += lut_div65535(x) != x / 65535u;
    return bad;
}

// one colour through steps 2 and 3 alone (the pixel function): Y and the 8-fold chroma of step 1 in, the table's R'G'B' out.  Returns 0, or -3
int emu_lut3d_pixel(const mihevc_lut3d_src *src, int n, const uint16_t *table, int Y, int cb8, int cr8, int *rgb16, int *looked_up)
{
    if (!lut3d_src_ok(src) || !lut3d_n_ok(n) || !table) return -3;
    std::unique_ptr<uint16_t[]> packed(new uint16_t[(size_t)n * n * n * 4]);
    lut3d_pack(n, table, packed.get());
    void *none[3] = {nullptr, nullptr, nullptr};
    const int stride[3] = {0, 0, 0};
    const Lut3dArgs a = lut3d_args(*src, n, packed.get(), nullptr, nullptr, nullptr, 0, 0, 16, 16, 16, 16, 8, 1, false, none, stride);
    lut_rgb16(a, Y, cb8, cr8, *(int(*)[3])rgb16);
    lut_lookup(a, *(int(*)[3])rgb16, *(int(*)[3])looked_up);
    return 0;
}

// src: the source's depth, matrix and range; table: n^3 x 3 uint16 in .cube order; y, u, v: tight source planes (pitch = row) of w x h / half-size samples, uint8 at
// depth 8, else uint16; out_*: tight planes of the coded size, uint8 at out_depth 8, uint16 at 10; order: SeqExec thread order; align: 16 / 8 / 4 / 1
// (IngestSrcPlane).  stats[0]: misaligned accesses (must be 0), stats[1]: samples written outside the coded width (must be 0), stats[2], stats[3]: the alignment
// class of the luma / chroma planes the kernel read.  Returns 0, or -3 for what mihevc_k_lut3d refuses
int emu_lut3d(const mihevc_lut3d_src *src, int n, const uint16_t *table, const void *y, const void *u, const void *v, int w, int h, int out_depth, int out_matrix,
              int out_full, int order, int align, void *out_y, void *out_u, void *out_v, int *stats)
{
    if (!lut3d_src_ok(src) || !lut3d_n_ok(n) || !table || !rgb_matrix_ok(out_matrix) || w < 16 || h < 16 || (w & 1) || (h & 1) || (out_depth != 8 && out_depth != 10)) return -3;
    if (align != 16 && align != 8 && align != 4 && align != 1) return -3;
    const void *p[3] = {y, u, v};
    void *out[3] = {out_y, out_u, out_v};
    const bool in16 = src->bit_depth > 8, out16 = out_depth > 8;
    if (in16 && out16) return run<uint16_t, uint16_t>(*src, n, table, p, w, h, out_depth, out_matrix, out_full, order, align, out, stats);
    if (in16) return run<uint16_t, uint8_t>(*src, n, table, p, w, h, out_depth, out_matrix, out_full, order, align, out, stats);
    if (out16) return run<uint8_t, uint16_t>(*src, n, table, p, w, h, out_depth, out_matrix, out_full, order, align, out, stats);
    return run<uint8_t, uint8_t>(*src, n, table, p, w, h, out_depth, out_matrix, out_full, order, align, out, stats);
}

}  // extern "C"
