// tests/emu/ingest.cpp — TEST HARNESS, NOT PRODUCT (part of tests/emu/libkernel_emu.so).  The source conversion program of hevc_amd/csrc/kernels/ingest.h (k_ingest)
// stepped on the CPU with the sequential executor, every workgroup of the launch.  The caller's tight planes are copied into source planes allocated to their
// exact size (they end with the last sample of the last row: a read past it is a finding of the AddressSanitizer program tests/test_ingest_cpu.py builds
// from this file and tests/ingest_asan_main.cc) with a pitch wider than
// the row and the alignment the case asks for; the output planes are filled with a garbage pattern first, so an unwritten sample shows, and the samples
// between the coded width and the stride must still hold it afterwards.  hevc_amd/ never loads this library.
#include "ingest_planes.h"
#include "../../hevc_amd/csrc/kernels/ingest.h"

using namespace mihevc;

namespace {

// align: the alignment class of the source planes (IngestSrcPlane)
template <typename TI, typename TO>
int run(const mihevc_src_format &f, const void *const *src, int w, int h, int out_depth, int order, int align, void *const *out, int *stats)
{
    const int pw = (w + 7) & ~7, ph = (h + 7) & ~7;
    IngestSrcPlane<TI> sp[3];
    for (int c = 0; c < (f.semi_planar ? 2 : 3); c++)
        if (!sp[c].place(src[c], c ? src_chroma_row(f, w) : w, c ? src_chroma_rows(f, h) : h, align)) return -5;
    IngestOutPlanes<TO> op(pw, ph);
    const IngestArgs a = ingest_args(f, sp[0].p, sp[1].p, sp[2].p, sp[0].pitch, sp[1].pitch, w, h, pw, ph, out_depth, op.dst, op.stride);
    stats[2] = a.align[0]; stats[3] = a.align[1];
    SeqExec ex;
    ex.order = order;
    g_ingest_misaligned = 0;
    const int nwg = ingest_workgroups(pw, ph, f.semi_planar);
    for (int wg = 0; wg < nwg; wg++) ingest_tile_program<TI, TO>(ex, a, wg);
    int wg_past = nwg;
    stats[0] = g_ingest_misaligned + (ingest_locate(pw, ph, f.semi_planar, wg_past) != -1);
    stats[1] = op.copy_back(out);
    return 0;
}

}  // namespace

extern "C" {

// the workgroup's tile in output samples: a test picks a size it does not divide
void emu_ingest_tile(int *tw, int *th) { *tw = ING_TW; *th = ING_TH; }

// fmt: a mihevc_src_format; y, u, v: tight source planes (pitch = row; semi-planar: u interleaved, v unused); w x h: display size; out_*: tight planes of the coded
// size, uint8 at out_depth 8, uint16 at 10; order: SeqExec thread order; align: 16 / 8 / 4 / 1 (IngestSrcPlane).  stats[0]: misaligned accesses (must be 0),
// stats[1]: samples written outside the coded width (must be 0), stats[2], stats[3]: the alignment class the kernel ran luma / chroma with.  Returns 0, or -3
int emu_ingest(const mihevc_src_format *fmt, const void *y, const void *u, const void *v, int w, int h, int out_depth, int order, int align, void *out_y, void *out_u,
               void *out_v, int *stats)
{
    if (!src_format_ok(fmt) || w < 16 || h < 16 || (w & 1) || (h & 1) || (out_depth != 8 && out_depth != 10)) return -3;
    if (align != 16 && align != 8 && align != 4 && align != 1) return -3;
    const void *src[3] = {y, u, v};
    void *out[3] = {out_y, out_u, out_v};
    const bool in16 = fmt->bit_depth > 8, out16 = out_depth > 8;
    if (in16 && out16) return run<uint16_t, uint16_t>(*fmt, src, w, h, out_depth, order, align, out, stats);
    if (in16) return run<uint16_t, uint8_t>(*fmt, src, w, h, out_depth, order, align, out, stats);
    if (out16) return run<uint8_t, uint16_t>(*fmt, src, w, h, out_depth, order, align, out, stats);
    return run<uint8_t, uint8_t>(*fmt, src, w, h, out_depth, order, align, out, stats);
}

}  // extern "C"
