// tests/emu/ingest_rgb.cpp — TEST HARNESS, NOT PRODUCT (part of tests/emu/libkernel_emu.so).  The RGB conversion program of hevc_amd/csrc/kernels/ingest_rgb.h
// (k_ingest_rgb) stepped on the CPU with the sequential executor, every workgroup of the launch.  As tests/emu/ingest.cpp: the caller's tight planes are copied
// into source planes allocated to their exact size (they end with the last sample of the last row: a read past it is a finding of the AddressSanitizer program
// tests/test_ingest_rgb_cpu.py builds from this file and tests/ingest_rgb_asan_main.cc), with a pitch wider than the row and the alignment the case asks for;
// the output planes are filled with a garbage pattern first, and the samples between the coded width and the stride must still hold it afterwards.
// hevc_amd/ never loads this library.
#include "ingest_planes.h"
#include "../../hevc_amd/csrc/kernels/ingest_rgb.h"

using namespace mihevc;

namespace {

// align: the alignment class of the source planes (IngestSrcPlane)
template <typename TI, bool FLT, typename TO>
int run(const mihevc_rgb_format &f, const void *const *src, int w, int h, int out_depth, int order, int align, void *const *out, int *stats)
{
    const int pw = (w + 7) & ~7, ph = (h + 7) & ~7;
    IngestSrcPlane<TI> sp[3];
    for (int c = 0; c < rgb_planes(f); c++)
        if (!sp[c].place(src[c], rgb_row_elems(f, w), h, align)) return -5;
    IngestOutPlanes<TO> op(pw, ph);
    const IngestRgbArgs a = ingest_rgb_args(f, f.matrix, f.range == 2, sp[0].p, sp[1].p, sp[2].p, sp[0].pitch, w, h, pw, ph, out_depth, op.dst, op.stride);
    stats[2] = a.align;
    SeqExec ex;
    ex.order = order;
    g_ingest_misaligned = 0;
    const int nwg = ingest_rgb_workgroups(pw, ph);
    for (int wg = 0; wg <= nwg; wg++) ingest_rgb_tile_program<TI, FLT, TO>(ex, a, wg);     // one past the last: writes nothing
    stats[0] = g_ingest_misaligned;
    stats[1] = op.copy_back(out);
    return 0;
}

template <typename TO>
int run_to(const mihevc_rgb_format &f, const void *const *src, int w, int h, int out_depth, int order, int align, void *const *out, int *stats)
{
    if (f.sample == 2) return run<uint32_t, true, TO>(f, src, w, h, out_depth, order, align, out, stats);
    if (f.sample == 1) return run<uint16_t, true, TO>(f, src, w, h, out_depth, order, align, out, stats);
    if (f.bit_depth > 8) return run<uint16_t, false, TO>(f, src, w, h, out_depth, order, align, out, stats);
    return run<uint8_t, false, TO>(f, src, w, h, out_depth, order, align, out, stats);
}

}  // namespace

extern "C" {

// the workgroup's tile in source pixels: a test picks a size it does not divide
void emu_ingest_rgb_tile(int *tw, int *th) { *tw = RGB_TW; *th = RGB_TH; }

// the integer coefficients of the host builder, R, G, B order: m[9] row by row, and S.  Returns 0, or -3 for an unknown matrix
int emu_ingest_rgb_matrix(int matrix, int full, int bits, int out_depth, int *m, int *S)
{
    int mm[3][3];
    if (!ingest_rgb_matrix(matrix, full != 0, bits, out_depth, mm, *S)) return -3;
    for (int i = 0; i < 9; i++) m[i] = mm[i / 3][i % 3];
    return 0;
}

// fmt: a mihevc_rgb_format with matrix and range explicit; p0 .. p2: tight source planes (pitch = row; packed: p0 only); w x h: display size; out_*: tight planes
// of the coded size, uint8 at out_depth 8, uint16 at 10; order: SeqExec thread order; align: 16 / 8 / 4 / 1 (IngestSrcPlane).  stats[0]: misaligned accesses (must
// be 0), stats[1]: samples written outside the coded width (must be 0), stats[2]: the alignment class the kernel ran with.  Returns 0, or -3
int emu_ingest_rgb(const mihevc_rgb_format *fmt, const void *p0, const void *p1, const void *p2, int w, int h, int out_depth, int order, int align, void *out_y,
                   void *out_u, void *out_v, int *stats)
{
    if (!rgb_format_ok(fmt) || !rgb_matrix_ok(fmt->matrix) || !fmt->range || w < 16 || h < 16 || (w & 1) || (h & 1) || (out_depth != 8 && out_depth != 10)) return -3;
    if (align != 16 && align != 8 && align != 4 && align != 1) return -3;
    const void *src[3] = {p0, p1, p2};
    void *out[3] = {out_y, out_u, out_v};
    if (out_depth > 8) return run_to<uint16_t>(*fmt, src, w, h, out_depth, order, align, out, stats);
    return run_to<uint8_t>(*fmt, src, w, h, out_depth, order, align, out, stats);
}

}  // extern "C"
