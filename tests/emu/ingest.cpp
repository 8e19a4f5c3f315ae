// tests/emu/ingest.cpp — TEST HARNESS, NOT PRODUCT (part of tests/emu/libkernel_emu.so).  The source conversion program of hevc_amd/csrc/kernels/ingest.h (k_ingest)
// stepped on the CPU with the sequential executor, every workgroup of the launch.  The caller's tight planes are copied into source planes allocated to their
// exact size (they end with the last sample of the last row: a read past it is a finding of the AddressSanitizer program tests/test_ingest_cpu.py builds
// from this file and tests/ingest_asan_main.cc) with a pitch wider than
// the row and the alignment the case asks for; the output planes are filled with a garbage pattern first, so an unwritten sample shows, and the samples
// between the coded width and the stride must still hold it afterwards.  hevc_amd/ never loads this library.
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

// the kernel header's access hook: chunk reads and stores whose address is not a multiple of their width
static int g_ingest_misaligned = 0;
#define MIHEVC_INGEST_ACCESS(p, bytes) ((void)(g_ingest_misaligned += ((uintptr_t)(p) % (unsigned)(bytes)) != 0))
#include "../../hevc_amd/csrc/kernels/ingest.h"

using namespace mihevc;

namespace {

// align: 16, 8, 4: the source planes' base address and pitch are multiples of it and of nothing larger; 1: base one element off, odd pitch
template <typename TI, typename TO>
int run(const mihevc_src_format &f, const void *const *src, int w, int h, int out_depth, int order, int align, void *const *out, int *stats)
{
    const int pw = (w + 7) & ~7, ph = (h + 7) & ~7;
    void *sbase[3] = {nullptr, nullptr, nullptr};
    const void *sp[3] = {nullptr, nullptr, nullptr};
    int pitch[3] = {0, 0, 0};
    for (int c = 0; c < (f.semi_planar ? 2 : 3); c++) {
        const int row = c ? src_chroma_row(f, w) : w, rows = c ? src_chroma_rows(f, h) : h;
        const int unit = align > 1 ? align / (int)sizeof(TI) : 1;                           // elements
        pitch[c] = ((row + unit - 1) / unit + 1) * unit;
        if (align < 16 && (pitch[c] / unit) % 2 == 0) pitch[c] += unit;                     // an odd multiple: not a multiple of the next power of two
        const size_t off = align == 16 ? 0 : align == 1 ? sizeof(TI) : (size_t)align;       // bytes from a 64-byte boundary
        const size_t bytes = ((size_t)pitch[c] * (rows - 1) + row) * sizeof(TI);
        if (posix_memalign(&sbase[c], 64, off + bytes)) return -5;                          // ends with the last sample of the last row
        memset(sbase[c], 0x5A, off + bytes);
        TI *p = (TI *)((uint8_t *)sbase[c] + off);
        for (int r = 0; r < rows; r++) memcpy(p + (size_t)r * pitch[c], (const TI *)src[c] + (size_t)r * row, (size_t)row * sizeof(TI));
        sp[c] = p;
    }
    constexpr TO kGarbage = (TO)0xA5A5;
    TO *op[3];
    void *obase[3];
    int ostride[3];
    for (int c = 0; c < 3; c++) {
        const int pwo = c ? pw / 2 : pw, pho = c ? ph / 2 : ph;
        ostride[c] = ((pwo + 15) & ~15) + 16;
        obase[c] = aligned_alloc(64, ((size_t)ostride[c] * pho * sizeof(TO) + 63) & ~(size_t)63);
        op[c] = (TO *)obase[c];
        for (size_t i = 0; i < (size_t)ostride[c] * pho; i++) op[c][i] = kGarbage;
    }
    void *dst[3] = {op[0], op[1], op[2]};
    const IngestArgs a = ingest_args(f, sp[0], sp[1], sp[2], pitch[0], pitch[1], w, h, pw, ph, out_depth, dst, ostride);
    stats[2] = a.align[0]; stats[3] = a.align[1];
    SeqExec ex;
    ex.order = order;
    g_ingest_misaligned = 0;
    const int nwg = ingest_workgroups(pw, ph, f.semi_planar);
    for (int wg = 0; wg < nwg; wg++) ingest_tile_program<TI, TO>(ex, a, wg);
    int wg_past = nwg;
    stats[0] = g_ingest_misaligned + (ingest_locate(pw, ph, f.semi_planar, wg_past) != -1);
    int spilled = 0;
    for (int c = 0; c < 3; c++) {
        const int pwo = c ? pw / 2 : pw, pho = c ? ph / 2 : ph;
        for (int r = 0; r < pho; r++) {
            memcpy((TO *)out[c] + (size_t)r * pwo, op[c] + (size_t)r * ostride[c], (size_t)pwo * sizeof(TO));
            for (int x = pwo; x < ostride[c]; x++) spilled += op[c][(size_t)r * ostride[c] + x] != kGarbage;
        }
        free(obase[c]);
        free(sbase[c]);
    }
    stats[1] = spilled;
    return 0;
}

}  // namespace

extern "C" {

// the workgroup's tile in output samples: a test picks a size it does not divide
void emu_ingest_tile(int *tw, int *th) { *tw = ING_TW; *th = ING_TH; }

// fmt: a mihevc_src_format; y, u, v: tight source planes (pitch = row; semi-planar: u interleaved, v unused); w x h: display size; out_*: tight planes of the coded
// size, uint8 at out_depth 8, uint16 at 10; order: SeqExec thread order; align: 16 / 8 / 4 / 1 (see run).  stats[0]: misaligned chunk accesses (must be 0),
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
