// tests/emu/fieldmatch.cpp — TEST HARNESS, NOT PRODUCT (part of tests/emu/libkernel_emu.so).  The programs of hevc_amd/csrc/kernels/fieldmatch.h (k_fm_metrics with
// k_fm_fold, k_fm_weave) stepped on the CPU with the sequential executor, every workgroup of a launch, and the planner of hevc_amd/csrc/fieldmatch_plan.h on plain
// arrays.  Source planes and output planes are those of the stepped converters (ingest_planes.h): sources allocated to their exact size with the alignment the
// case asks for (a read past them is a finding of the AddressSanitizer program tests/test_fieldmatch_cpu.py builds from this file and
// tests/fieldmatch_asan_main.cc), outputs garbage-filled.  A workgroup's LDS image starts as pseudo-random bytes (lds_seed), as it does on the device, and so do the
// partials.  hevc_amd/ never loads this library.
#include <memory>
#include <vector>

#include "ingest_planes.h"
#include "../../hevc_amd/csrc/kernels/fieldmatch.h"
#include "../../hevc_amd/csrc/fieldmatch_plan.h"

using namespace mihevc;

namespace {

struct Garbage {
    unsigned long long x;
    explicit Garbage(unsigned seed) : x(0x9E3779B97F4A7C15ull ^ seed) {}
    void fill(void *p, size_t n)
    {
        unsigned char *b = (unsigned char *)p;
        for (size_t i = 0; i < n; i++) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; b[i] = (unsigned char)(x >> 32); }
    }
};

template <typename T>
int run_metrics(const void *prev, const void *cur, const void *next, int w, int h, int depth, int keep, int order, int align, unsigned lds_seed, unsigned long long *out, int *stats)
{
    IngestSrcPlane<T> sp[3];
    const void *src[3] = {prev, cur, next};
    for (int f = 0; f < 3; f++)
        if (!sp[f].place(src[f], w, h, align)) return -5;
    const int nwg = fm_workgroups(w, h);
    std::vector<unsigned long long> part((size_t)nwg * 8);
    Garbage g(lds_seed);
    g.fill(part.data(), part.size() * sizeof(unsigned long long));
    const FmArgs a = fm_args(depth, sp[0].p, sp[1].p, sp[2].p, sp[0].pitch, w, h, keep, part.data());
    stats[2] = a.align;
    SeqExec ex;
    ex.order = order;
    g_ingest_misaligned = 0;
    std::unique_ptr<FmShared> sh(new FmShared);
    for (int wg = 0; wg < nwg + 1; wg++) {          // (one past the last: it must do nothing)
        g.fill(sh.get(), sizeof(FmShared));
        fm_metrics_program<T>(ex, *sh, a, wg);
    }
    g.fill(sh.get(), sizeof(FmShared));
    fm_fold_program(ex, *sh, part.data(), nwg, out);
    stats[0] = g_ingest_misaligned;
    stats[1] = 0;
    return 0;
}

template <typename T>
int run_weave(const void *const *cur, const void *const *other, int w, int h, int depth, int keep, int order, int align, void *const *out, int *stats)
{
    const int pw = (w + 7) & ~7, ph = (h + 7) & ~7;
    IngestSrcPlane<T> sp[2][3];
    const void *p[2][3];
    for (int f = 0; f < 2; f++)
        for (int c = 0; c < 3; c++) {
            if (!sp[f][c].place((f ? other : cur)[c], c ? w / 2 : w, c ? h / 2 : h, align)) return -5;
            p[f][c] = sp[f][c].p;
        }
    IngestOutPlanes<T> op(pw, ph);
    const DeintArgs a = deint_args(depth, p[1], p[0], p[1], sp[0][0].pitch, sp[0][1].pitch, w, h, pw, ph, keep, 0, op.dst, op.stride);
    stats[2] = a.align[0]; stats[3] = a.align[1];
    SeqExec ex;
    ex.order = order;
    g_ingest_misaligned = 0;
    const int nwg = deint_workgroups(pw, ph);
    for (int wg = 0; wg < nwg + 1; wg++) fm_weave_program<T>(ex, a, wg);
    stats[0] = g_ingest_misaligned;
    stats[1] = op.copy_back(out);
    return 0;
}

bool fm_case_ok(int w, int h, int depth, int keep, int align)
{
    return deint_geometry_ok(w, h) && (depth == 8 || depth == 10) && (keep == 0 || keep == 1) && (align == 16 || align == 8 || align == 4 || align == 1);
}

}  // namespace

extern "C" {

// the metrics tile in luma samples and the bytes of the workgroup's LDS
void emu_fm_tile(int *tw, int *th, int *lds_bytes) { *tw = FM_TW; *th = FM_TH; *lds_bytes = (int)sizeof(FmShared); }

// prev / cur / next: luma of three frames of w x h samples as tight planes, uint8 at depth 8, uint16 at 10; out: S_c S_p S_n K_c K_p K_n DS DB; order: SeqExec
// thread order; align: 16 / 8 / 4 / 1 (IngestSrcPlane); lds_seed: of the garbage.  stats[0]: misaligned accesses (must be 0), stats[2]: the alignment class the
// kernel read the planes with.  Returns 0, or -3 for what mihevc_k_fieldmatch_metrics refuses
int emu_fm_metrics(const void *prev, const void *cur, const void *next, int w, int h, int depth, int keep, int order, int align, unsigned lds_seed,
                   unsigned long long *out, int *stats)
{
    if (!fm_case_ok(w, h, depth, keep, align)) return -3;
    if (depth > 8) return run_metrics<uint16_t>(prev, cur, next, w, h, depth, keep, order, align, lds_seed, out, stats);
    return run_metrics<uint8_t>(prev, cur, next, w, h, depth, keep, order, align, lds_seed, out, stats);
}

// cur / other: Y, Cb, Cr of the frame that gives the rows of parity keep and of the frame that gives the others, tight planes; out_*: tight planes of the coded
// size.  stats[0]: misaligned accesses, stats[1]: samples written outside the coded width (both must be 0), stats[2], stats[3]: the alignment class of the luma /
// chroma planes the kernel read.  Returns 0, or -3 for what mihevc_k_fieldmatch_weave refuses
int emu_fm_weave(const void *const *cur, const void *const *other, int w, int h, int depth, int keep, int order, int align, void *out_y, void *out_u, void *out_v,
                 int *stats)
{
    if (!fm_case_ok(w, h, depth, keep, align)) return -3;
    void *out[3] = {out_y, out_u, out_v};
    if (depth > 8) return run_weave<uint16_t>(cur, other, w, h, depth, keep, order, align, out, stats);
    return run_weave<uint8_t>(cur, other, w, h, depth, keep, order, align, out, stats);
}

// A whole clip at once, with the planner's functions called as a session calls them frame by frame.  metrics: n x 8 numbers as k_fm_fold leaves them (the first
// frame's all-ones are set here).  match, fallback, dropped, picture (the output index, -1 dropped): room for n.  Returns the number of pictures
long long emu_fm_plan(const unsigned long long *metrics, int n, int decimate, int deint, int *match, int *fallback, int *dropped, long long *picture)
{
    std::vector<FmMetrics> m((size_t)n);
    for (int k = 0; k < n; k++) {
        m[(size_t)k] = fm_metrics_of(metrics + (size_t)k * 8);
        if (k == 0) fm_first_frame(m[0]);
        match[k] = fm_match(m[(size_t)k]);
        fallback[k] = fm_falls_back(m[(size_t)k], match[k], deint != 0);
    }
    long long pictures = 0;
    for (int k0 = 0; k0 < n; k0 += kFmCycle) {
        const int drop = decimate && k0 + kFmCycle <= n ? k0 + fm_drop(m.data() + k0) : -1;      // (a last cycle with fewer frames drops nothing)
        for (int k = k0; k < n && k < k0 + kFmCycle; k++) {
            dropped[k] = k == drop;
            picture[k] = k == drop ? -1 : pictures++;
        }
    }
    return pictures;
}

}  // extern "C"
