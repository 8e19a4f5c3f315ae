// tests/emu/scale.cpp — TEST HARNESS, NOT PRODUCT (part of tests/emu/libkernel_emu.so).  The downscaling program of hevc_amd/csrc/kernels/scale.h (k_scale) stepped
// on the CPU with the sequential executor, every workgroup of the launch, over the tables of hevc_amd/csrc/scale_taps.h, which it also hands out as they are.
// Source planes and output planes are those of the stepped converters (ingest_planes.h): sources allocated to their exact size with the alignment the case
// asks for (a read past them is a finding of the AddressSanitizer program tests/test_scale_cpu.py builds from this file and tests/scale_asan_main.cc),
// outputs garbage-filled.  The workgroup's LDS image starts as pseudo-random bytes (lds_seed), as it does on the device.  hevc_amd/ never loads this library.
#include <memory>
#include <vector>

#include "ingest_planes.h"
#include "../../hevc_amd/csrc/kernels/scale.h"
#include "../../hevc_amd/csrc/scale_taps.h"

using namespace mihevc;

namespace {

template <typename TI, typename TO>
int run(const mihevc_scale_src &f, const void *const *src, int dw, int dh, int out_depth, int order, int align, unsigned lds_seed, void *const *out, int *stats)
{
    const int pw = (dw + 7) & ~7, ph = (dh + 7) & ~7;
    ScaleBlock blk;
    if (!scale_block_build(f.width, f.height, dw, dh, SC_TH, SC_ROWS, blk)) return -3;
    IngestSrcPlane<TI> sp[3];
    for (int c = 0; c < 3; c++)
        if (!sp[c].place(src[c], c ? f.width / 2 : f.width, c ? f.height / 2 : f.height, align)) return -5;
    IngestOutPlanes<TO> op(pw, ph);
    const int32_t *first[4];
    const int16_t *coef[4];
    for (int k = 0; k < 4; k++) { first[k] = (const int32_t *)(blk.bytes.data() + blk.first[k]); coef[k] = (const int16_t *)(blk.bytes.data() + blk.coef[k]); }
    const ScaleArgs a = scale_args(f.bit_depth, sp[0].p, sp[1].p, sp[2].p, sp[0].pitch, sp[1].pitch, f.width, f.height, dw, dh, pw, ph, out_depth, op.dst, op.stride,
                                   first, coef, blk.taps);
    stats[2] = ingest_align(a.src[0], (size_t)a.pitch[0] * sizeof(TI)); stats[3] = ingest_align(a.src[1], (size_t)a.pitch[1] * sizeof(TI));
    SeqExec ex;
    ex.order = order;
    g_ingest_misaligned = 0;
    std::unique_ptr<ScaleShared> sh(new ScaleShared);
    unsigned long long x = 0x9E3779B97F4A7C15ull ^ lds_seed;
    const int nwg = scale_workgroups(pw, ph);
    for (int wg = 0; wg < nwg; wg++) {
        unsigned char *b = (unsigned char *)sh.get();
        for (size_t i = 0; i < sizeof(ScaleShared); i++) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; b[i] = (unsigned char)(x >> 32); }
        scale_tile_program<TI, TO>(ex, *sh, a, wg);
    }
    int wg_past = nwg;
    stats[0] = g_ingest_misaligned + (scale_locate(pw, ph, wg_past) != -1);
    stats[1] = op.copy_back(out);
    return 0;
}

}  // namespace

extern "C" {

// the workgroup's tile in output samples and the rows of its LDS image: a test picks sizes the tile does not divide
void emu_scale_tile(int *tw, int *th, int *rows) { *tw = SC_TW; *th = SC_TH; *rows = SC_ROWS; }

// scale_taps_build(S, Dn, p): first[Dn], coef[Dn * 16], *taps.  Returns 0, or -3 when the builder refuses
int emu_scale_taps(int S, int Dn, int p, int32_t *first, int16_t *coef, int *taps)
{
    ScaleTaps t;
    if (!scale_taps_build(S, Dn, p, t)) return -3;
    memcpy(first, t.first.data(), t.first.size() * sizeof(int32_t));
    memcpy(coef, t.coef.data(), t.coef.size() * sizeof(int16_t));
    *taps = t.taps;
    return 0;
}

// src: the source's size and depth; y, u, v: its tight planes (pitch = row); dw x dh: display size of the output; out_*: tight planes of the coded size, uint8 at
// out_depth 8, uint16 at 10; order: SeqExec thread order; align: 16 / 8 / 4 / 1 (IngestSrcPlane); lds_seed: of the LDS image's initial bytes.  stats[0]:
// misaligned accesses (must be 0), stats[1]: samples written outside the coded width (must be 0), stats[2], stats[3]: the alignment class of the luma / chroma
// planes the kernel read.  Returns 0, or -3
int emu_scale(const mihevc_scale_src *src, const void *y, const void *u, const void *v, int dw, int dh, int out_depth, int order, int align, unsigned lds_seed,
              void *out_y, void *out_u, void *out_v, int *stats)
{
    if (!scale_src_ok(src) || !scale_geometry_ok(src->width, src->height, dw, dh) || (out_depth != 8 && out_depth != 10)) return -3;
    if (align != 16 && align != 8 && align != 4 && align != 1) return -3;
    const void *p[3] = {y, u, v};
    void *out[3] = {out_y, out_u, out_v};
    const bool in16 = src->bit_depth > 8, out16 = out_depth > 8;
    if (in16 && out16) return run<uint16_t, uint16_t>(*src, p, dw, dh, out_depth, order, align, lds_seed, out, stats);
    if (in16) return run<uint16_t, uint8_t>(*src, p, dw, dh, out_depth, order, align, lds_seed, out, stats);
    if (out16) return run<uint8_t, uint16_t>(*src, p, dw, dh, out_depth, order, align, lds_seed, out, stats);
    return run<uint8_t, uint8_t>(*src, p, dw, dh, out_depth, order, align, lds_seed, out, stats);
}

}  // extern "C"
