// tests/emu/mcfi.cpp — TEST HARNESS, NOT PRODUCT (part of tests/emu/libkernel_emu.so).  The programs of hevc_amd/csrc/kernels/mcfi.h (k_mcfi_search, k_mcfi_field,
// k_mcfi_render) stepped on the CPU with the sequential executor, every workgroup of each launch.  Source planes and output planes are those of the stepped
// converters (ingest_planes.h): the source planes allocated to their exact size with the alignment the case asks for (a read past them is a finding of the
// AddressSanitizer program tests/test_mcfi_cpu.py builds from this file and tests/mcfi_asan_main.cc), outputs garbage-filled.  The workgroup's LDS images and the
// device block (vectors, SAD0(0), parts of D) start as pseudo-random bytes (lds_seed), as they do on the device.  hevc_amd/ never loads this library.
#include <memory>
#include <vector>

#include "ingest_planes.h"
#include "../../hevc_amd/csrc/kernels/mcfi.h"

using namespace mihevc;

namespace {

struct Noise {
    unsigned long long x;
    explicit Noise(unsigned seed) : x(0x9E3779B97F4A7C15ull ^ seed) {}
    void fill(void *p, size_t n)
    {
        unsigned char *b = (unsigned char *)p;
        for (size_t i = 0; i < n; i++) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; b[i] = (unsigned char)(x >> 32); }
    }
};

template <typename T>
int run_vectors(const void *cur, const void *next, int w, int h, int depth, int order, int align, unsigned lds_seed, int16_t *v0, int16_t *v, uint64_t *scene_sum, int *stats)
{
    IngestSrcPlane<T> sp[2];
    if (!sp[0].place(cur, w, h, align) || !sp[1].place(next, w, h, align)) return -5;
    const McfiLayout l = mcfi_layout(w, h);
    std::vector<unsigned long long> blk((l.bytes + 7) / 8);
    Noise nz(lds_seed);
    nz.fill(blk.data(), l.bytes);
    const McfiSearchArgs a = mcfi_search_args(depth, sp[0].p, sp[1].p, sp[0].pitch, w, h, (uint8_t *)blk.data());
    const McfiFieldArgs f = mcfi_field_args(a, (uint8_t *)blk.data());
    stats[2] = a.align;
    SeqExec ex;
    ex.order = order;
    g_ingest_misaligned = 0;
    std::unique_ptr<McfiSearchShared> ss(new McfiSearchShared);
    for (int wg = 0; wg <= mcfi_search_workgroups(w, h); wg++) {      // (one past the last: it must do nothing)
        nz.fill(ss.get(), sizeof(McfiSearchShared));
        mcfi_search_program<T>(ex, *ss, a, wg);
    }
    std::unique_ptr<McfiFieldShared> fs(new McfiFieldShared);
    for (int wg = 0; wg <= mcfi_field_workgroups(w, h); wg++) {
        nz.fill(fs.get(), sizeof(McfiFieldShared));
        mcfi_field_program<T>(ex, *fs, f, wg);
    }
    stats[0] = g_ingest_misaligned;
    const size_t nb = (size_t)a.nbx * a.nby;
    memcpy(v0, a.v0, nb * 4);
    memcpy(v, f.v, nb * 4);
    *scene_sum = *f.dsum;
    return 0;
}

template <typename T>
int run_render(const mihevc_interpolate &m, int j, const void *const *cur, const void *const *next, const int16_t *v, uint64_t scene_sum, int w, int h, int depth, int order,
               int align, unsigned lds_seed, void *const *out, int *stats)
{
    const int pw = (w + 7) & ~7, ph = (h + 7) & ~7;
    IngestSrcPlane<T> sp[2][3];
    const void *p[2][3];
    for (int f = 0; f < 2; f++)
        for (int c = 0; c < 3; c++) {
            if (!sp[f][c].place((f ? next : cur)[c], c ? w / 2 : w, c ? h / 2 : h, align)) return -5;
            p[f][c] = sp[f][c].p;
        }
    IngestOutPlanes<T> op(pw, ph);
    const unsigned long long sum = scene_sum;
    const McfiRenderArgs a = mcfi_render_args(m, j, depth, p[0], p[1], sp[0][0].pitch, sp[0][1].pitch, w, h, pw, ph, v, &sum, op.dst, op.stride);
    stats[2] = a.align[0]; stats[3] = a.align[1];
    SeqExec ex;
    ex.order = order;
    g_ingest_misaligned = 0;
    Noise nz(lds_seed);
    std::unique_ptr<McfiRenderShared> sh(new McfiRenderShared);
    for (int wg = 0; wg <= mcfi_render_workgroups(pw, ph); wg++) {
        nz.fill(sh.get(), sizeof(McfiRenderShared));
        mcfi_render_program<T>(ex, *sh, a, wg);
    }
    stats[0] = g_ingest_misaligned;
    stats[1] = op.copy_back(out);
    return 0;
}

}  // namespace

extern "C" {

// blocks of a search tile's side, the render tile in output samples, and the bytes of the three LDS images
void emu_mcfi_tiles(int *search_blocks, int *render_tw, int *render_th, int *lds_bytes)
{
    *search_blocks = MC_SB; *render_tw = MR_TW; *render_th = MR_TH;
    lds_bytes[0] = (int)sizeof(McfiSearchShared); lds_bytes[1] = (int)sizeof(McfiFieldShared); lds_bytes[2] = (int)sizeof(McfiRenderShared);
}

// the kernel's own output division (mcfi_div) against the language's over the whole numerator range of the definition, 0 <= num < 2^23, for f = 2, 3, 4, and
// its offset division (mcfi_q) for every d = 2v, |v| <= 18, and every j < f.  Returns the number of wrong results
int emu_mcfi_div_check()
{
    int bad = 0;
    for (int f = 2; f <= 4; f++) {
        for (int num = 0; num < (1 << 23); num++) bad += mcfi_div(num, f) != (num + 512 * f) / (1024 * f);
        for (int d = -2 * MC_VMAX; d <= 2 * MC_VMAX; d += 2)
            for (int j = 0; j < f; j++) {
                const int n = 8 * d * j + f, q = n >= 0 ? n / (2 * f) : -((-n + 2 * f - 1) / (2 * f));
                bad += mcfi_q(d, j, f) != q;
            }
    }
    return bad;
}

// cur_y / next_y: luma of two frames of w x h samples as tight planes (pitch = row), uint8 at depth 8, uint16 at 10; v0 / v: ceil(h / 8) x ceil(w / 8) pairs;
// order: SeqExec thread order; align: 16 / 8 / 4 / 1 (IngestSrcPlane); lds_seed: of the initial bytes of LDS and of the device block.  stats[0]: misaligned
// accesses (must be 0), stats[2]: the alignment class the kernel read with.  Returns 0, or -3 for what mihevc_k_mcfi_vectors refuses
int emu_mcfi_vectors(const void *cur_y, const void *next_y, int w, int h, int depth, int order, int align, unsigned lds_seed, int16_t *v0, int16_t *v, uint64_t *scene_sum,
                     int *stats)
{
    if (!mcfi_geometry_ok(w, h) || (depth != 8 && depth != 10) || (align != 16 && align != 8 && align != 4 && align != 1)) return -3;
    if (depth > 8) return run_vectors<uint16_t>(cur_y, next_y, w, h, depth, order, align, lds_seed, v0, v, scene_sum, stats);
    return run_vectors<uint8_t>(cur_y, next_y, w, h, depth, order, align, lds_seed, v0, v, scene_sum, stats);
}

// cur / next: Y, Cb, Cr of two frames as tight planes; v: the caller's field (NULL under blend); out_*: tight planes of the coded size.  stats[0]: misaligned
// accesses, stats[1]: samples written outside the coded width (both must be 0), stats[2], stats[3]: the alignment class of the luma / chroma planes.  Returns 0,
// or -3 for what mihevc_k_mcfi_render refuses
int emu_mcfi_render(const mihevc_interpolate *m, int j, const void *const *cur, const void *const *next, const int16_t *v, uint64_t scene_sum, int w, int h, int depth,
                    int order, int align, unsigned lds_seed, void *out_y, void *out_u, void *out_v, int *stats)
{
    if (!mcfi_mode_ok(m) || j < 0 || j >= m->factor || !mcfi_geometry_ok(w, h) || (depth != 8 && depth != 10) || (!v && m->mode == 0)) return -3;
    if (v && !mcfi_vectors_ok(v, (size_t)mcfi_blocks(w) * mcfi_blocks(h))) return -3;
    if (align != 16 && align != 8 && align != 4 && align != 1) return -3;
    void *out[3] = {out_y, out_u, out_v};
    if (depth > 8) return run_render<uint16_t>(*m, j, cur, next, v, scene_sum, w, h, depth, order, align, lds_seed, out, stats);
    return run_render<uint8_t>(*m, j, cur, next, v, scene_sum, w, h, depth, order, align, lds_seed, out, stats);
}

}  // extern "C"
