// hevc_amd/csrc/device.hip — __global__ entry points, launchers and the per-stage C-ABI functions (mihevc_k_*).
#include "device.h"
#include "md5.h"
#include "scale_taps.h"
#include "stage_args.h"

#include <cstdio>
#include <cstring>
#include <vector>

namespace mihevc {

__host__ __device__ static inline size_t round16(size_t v) { return (v + 15) & ~(size_t)15; }

// XCD-aware block -> CTU map: blocks b and b+8 share an XCD (and its L2), so give each XCD one contiguous run of
// CTUs; neighbouring CTUs overlap in their search windows (MI355X_MICROARCH.md, workgroup dispatch).
__device__ __forceinline__ int xcd_remap(int b, int n)
{
    int chunk = (n + 7) >> 3;
    return (b & 7) * chunk + (b >> 3);
}

// list 1: the search of a B picture against the anchor after it (InterArgs::ref1 / centers1 / me1).  RANGE: me_range as a compile-time constant
// (15, the default of a session: launch_me_search picks it) or 0 for any range (me_search_program)
template <typename T, int RANGE> __global__ __launch_bounds__(NT, 5) void k_me_search(const InterArgs<T> *args, int n_ctu, int list)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int ctu = xcd_remap(blockIdx.x, n_ctu);
    if (ctu >= n_ctu) return;
    MeShared<T> &s = *reinterpret_cast<MeShared<T> *>(smem);
    uint8_t *win = smem + round16(sizeof(MeShared<T>));
    GpuExec ex;
    if (list) {
        const InterArgs<T> a = list1_view(args[blockIdx.y]);
        me_search_program<T, RANGE>(ex, s, win, a, ctu);
    } else me_search_program<T, RANGE>(ex, s, win, args[blockIdx.y], ctu);
}

// 5 workgroups per CU at 8 bit (89 VGPRs, no scratch; the windows overlay the residual area, inter_lds: 31,440 B of LDS at me_range 15), 3 at
// 10 bit (LDS).  Y_IN: the luma window lies in rs.scratch (inter_lds); its offset is a compile-time constant either way.  From a runtime base the
// compiler merges the window's 4-byte-aligned dword reads into ds_read_b128 / b96, mostly misaligned, and the LDS replays them
// (SQ_LDS_UNALIGNED_STALL 2.8e7 -> 9.7e7 per launch against the ds_read2_b32 pairs of a constant base, DESIGN.md §6a')
template <typename T, bool Y_IN> __global__ __launch_bounds__(NT, (sizeof(T) == 1 ? 5 : 4)) void k_inter_ctu(const InterArgs<T> *args, int n_ctu)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int ctu = xcd_remap(blockIdx.x, n_ctu);
    if (ctu >= n_ctu) return;
    const InterArgs<T> &a = args[blockIdx.y];
    const InterLds l = inter_lds<T>(a.prm.me_range);
    InterShared<T> &s = *reinterpret_cast<InterShared<T> *>(smem);
    T *wy = reinterpret_cast<T *>(smem + (Y_IN ? inter_win_in<T>() : inter_win_out<T>()));
    GpuExec ex;
    inter_ctu_program<T>(ex, s, wy, reinterpret_cast<T *>(smem + l.u), reinterpret_cast<T *>(smem + l.v), a, ctu);
}

// B pictures: the same CTU program with the list-1 refinement and the bi-prediction trial (BiShared sits behind the windows); 3 workgroups per CU
template <typename T> __global__ __launch_bounds__(NT, 3) void k_inter_ctu_b(const InterArgs<T> *args, int n_ctu)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int ctu = xcd_remap(blockIdx.x, n_ctu);
    if (ctu >= n_ctu) return;
    const InterArgs<T> &a = args[blockIdx.y];
    const InterBLds l = inter_b_lds<T>(a.prm.me_range);
    InterShared<T> &s = *reinterpret_cast<InterShared<T> *>(smem);
    GpuExec ex;
    inter_ctu_program<T, GpuExec, true>(ex, s, reinterpret_cast<T *>(smem + l.y), reinterpret_cast<T *>(smem + l.u), reinterpret_cast<T *>(smem + l.v), a, ctu,
                                        reinterpret_cast<BiShared *>(smem + l.bi));
}

// stage A of the intra pictures: every CTU of every picture in flight plans its quadtree and modes on the source picture (kernels/intra.h);
// a throughput kernel like k_inter_ctu: 3 workgroups per CU fit its 50 KB of LDS (8 bit)
#ifndef INTRA_OCC
#define INTRA_OCC 3
#endif
template <typename T> __global__ __launch_bounds__(NT, (sizeof(T) == 1 ? INTRA_OCC : 2)) void k_intra_plan(const IntraArgs<T> *args, int n_ctu)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int ctu = xcd_remap(blockIdx.x, n_ctu);
    if (ctu >= n_ctu) return;
    const IntraArgs<T> &a = args[blockIdx.y];
    IntraShared<T> &s = *reinterpret_cast<IntraShared<T> *>(smem);
    GpuExec ex;
    intra_plan_program<T>(ex, s, a, ctu % a.ctus_w, ctu / a.ctus_w);
}

// stage B: blockIdx.x = tile * rows_per_tile + row inside the tile: every tile row holds at most one CTU of a diagonal.  A launch holds
// few hundred CTU programs (pictures x tiles x rows), each a chain of barrier phases: latency bound, so the planned CUs are all it runs
template <typename T> __global__ __launch_bounds__(NT, 2) void k_intra_diag(const IntraArgs<T> *args, int diagonal, int rows_per_tile)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const IntraArgs<T> &a = args[blockIdx.y];
    const int tcn = a.prm.tile_cols > 1 ? a.prm.tile_cols : 1, trn = a.prm.tile_rows > 1 ? a.prm.tile_rows : 1;
    const int tile = (int)blockIdx.x / rows_per_tile, r = (int)blockIdx.x % rows_per_tile;
    if (tile >= tcn * trn) return;
    const int tx = tile % tcn, ty = tile / tcn;
    const int cx0 = tile_bd(tx, tcn, a.ctus_w), cx1 = tile_bd(tx + 1, tcn, a.ctus_w), cy0 = tile_bd(ty, trn, a.ctus_h), cy1 = tile_bd(ty + 1, trn, a.ctus_h);
    const int cy = cy0 + r, cx = cx0 + diagonal - 2 * r;
    if (cy >= cy1 || cx < cx0 || cx >= cx1) return;
    IntraShared<T> &s = *reinterpret_cast<IntraShared<T> *>(smem);
    GpuExec ex;
    intra_code_program<T>(ex, s, a, cx, cy, true);
}

template <typename T> __global__ __launch_bounds__(256) void k_lowres(const PreArgs<T> *args)
{
    lowres_sample<T>(args[blockIdx.y], (int)(blockIdx.x * 256 + threadIdx.x));
}
template <typename T> __global__ __launch_bounds__(NT) void k_pre_search(const PreArgs<T> *args, int n_ctu)
{
    __shared__ __align__(16) PreShared s;
    if ((int)blockIdx.x >= n_ctu) return;
    GpuExec ex;
    pre_search_program<T>(ex, s, args[blockIdx.y], (int)blockIdx.x);
}

// intra second pass of P pictures: one workgroup per CTU, most of them leave at once (not a candidate of this round)
template <typename T> __global__ __launch_bounds__(NT, 2) void k_intra_p(const IntraArgs<T> *args, int n_ctu, int round)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const IntraArgs<T> &a = args[blockIdx.y];
    const int ctu = (int)blockIdx.x;
    if (ctu >= n_ctu || !a.ip) return;
    const int cx = ctu % a.ctus_w, cy = ctu / a.ctus_w;
    if (!ip_eligible(a.ip, a.ctus_w, a.ctus_h, cx, cy, round)) return;
    IntraShared<T> &s = *reinterpret_cast<IntraShared<T> *>(smem);
    GpuExec ex;
    intra_ctu_program<T>(ex, s, a, cx, cy);
}

template <typename T> __global__ __launch_bounds__(256) void k_deblock(const DeblockArgs<T> *args)
{
    deblock_segment<T>(args[blockIdx.y], blockIdx.x * 256 + threadIdx.x);
}

// 8 workgroups per CU = every wave slot (49 / 55 VGPRs, 17 / 21 KB of LDS at 8 / 10 bit: the 10-bit form fits 7)
template <typename T> __global__ __launch_bounds__(NT, (sizeof(T) == 1 ? 8 : 7)) void k_sao_decide(const SaoArgs<T> *args, int n_ctu)
{
    __shared__ SaoShared<T> s;
    const int ctu = xcd_remap(blockIdx.x, n_ctu);
    if (ctu >= n_ctu) return;
    const SaoArgs<T> &a = args[blockIdx.y];
    GpuExec ex;
    sao_ctu_program<T>(ex, s, a, ctu);
}

// one thread per four samples of a row; rows of a plane are walked by consecutive lanes (coalesced dword / qword accesses)
template <typename T> __global__ __launch_bounds__(256) void k_sao_apply(const SaoArgs<T> *args)
{
    const SaoArgs<T> &a = args[blockIdx.y];
    const int ql = (a.w * a.h) >> 2, qc = ql >> 2, qwl = a.w >> 2, qwc = a.w >> 3;
    int i = blockIdx.x * 256 + threadIdx.x;
    if (i < ql) { sao_apply_quad<T>(a, 0, (i % qwl) * 4, i / qwl); return; }
    i -= ql;
    if (i < qc) { sao_apply_quad<T>(a, 1, (i % qwc) * 4, i / qwc); return; }
    i -= qc;
    if (i < qc) sao_apply_quad<T>(a, 2, (i % qwc) * 4, i / qwc);
}

template <typename T> __global__ __launch_bounds__(256) void k_pad(const SaoArgs<T> *args)
{
    const SaoArgs<T> &a = args[blockIdx.y];
    const int ny = pad_border_quads(a.w, a.h, PAD_Y), ncp = pad_border_quads(a.w >> 1, a.h >> 1, PAD_C);      // border only, four samples a lane
    int i = blockIdx.x * 256 + threadIdx.x;
    if (i < ny) { pad_border_quad<T>(a.out[0], a.w, a.h, PAD_Y, i); return; }
    i -= ny;
    if (i < ncp) { pad_border_quad<T>(a.out[1], a.w >> 1, a.h >> 1, PAD_C, i); return; }
    i -= ncp;
    if (i < ncp) pad_border_quad<T>(a.out[2], a.w >> 1, a.h >> 1, PAD_C, i);
}

// fill the coded-size margin of a source plane (columns sw..pw-1, rows sh..ph-1) by edge replication
template <typename T> __global__ __launch_bounds__(256) void k_extend_margin(Plane<T> p, int sw, int sh, int pw, int ph)
{
    int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= pw * ph) return;
    int x = i % pw, y = i / pw;
    if (x < sw && y < sh) return;
    p.p[(ptrdiff_t)y * p.stride + x] = p.p[(ptrdiff_t)(y < sh ? y : sh - 1) * p.stride + (x < sw ? x : sw - 1)];
}
template <typename T> hipError_t launch_extend_margin(hipStream_t st, Plane<T> p, int sw, int sh, int pw, int ph)
{
    hipLaunchKernelGGL(k_extend_margin<T>, dim3((unsigned)((pw * ph + 255) / 256)), dim3(256), 0, st, p, sw, sh, pw, ph);
    return hipGetLastError();
}

// source conversion (kernels/ingest.h): one workgroup per tile of output samples, Y, then Cb, then Cr; the argument block travels by value
template <typename TI, typename TO> __global__ __launch_bounds__(NT) void k_ingest(const IngestArgs a)
{
    GpuExec ex;
    ingest_tile_program<TI, TO>(ex, a, (int)blockIdx.x);
}
hipError_t launch_ingest(hipStream_t st, const IngestArgs &a, bool in16, bool out16)
{
    const dim3 grid((unsigned)ingest_workgroups(a.pw, a.ph, a.semi)), block(NT);
    if (in16 && out16) hipLaunchKernelGGL((k_ingest<uint16_t, uint16_t>), grid, block, 0, st, a);
    else if (in16) hipLaunchKernelGGL((k_ingest<uint16_t, uint8_t>), grid, block, 0, st, a);
    else if (out16) hipLaunchKernelGGL((k_ingest<uint8_t, uint16_t>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_ingest<uint8_t, uint8_t>), grid, block, 0, st, a);
    return hipGetLastError();
}

// downscaling source (kernels/scale.h): one workgroup per tile of SC_TW x SC_TH output samples, Y, then Cb, then Cr; the argument block travels by value.
// 40,960 bytes of LDS and 72 / 74 VGPRs: four workgroups per CU (4 waves per SIMD), which take the CU's 160 KB of LDS exactly
template <typename TI, typename TO> __global__ __launch_bounds__(NT, 4) void k_scale(const ScaleArgs a)
{
    __shared__ __align__(16) ScaleShared s;
    GpuExec ex;
    scale_tile_program<TI, TO>(ex, s, a, (int)blockIdx.x);
}
hipError_t launch_scale(hipStream_t st, const ScaleArgs &a, bool in16, bool out16)
{
    const dim3 grid((unsigned)scale_workgroups(a.pw, a.ph)), block(NT);
    if (in16 && out16) hipLaunchKernelGGL((k_scale<uint16_t, uint16_t>), grid, block, 0, st, a);
    else if (in16) hipLaunchKernelGGL((k_scale<uint16_t, uint8_t>), grid, block, 0, st, a);
    else if (out16) hipLaunchKernelGGL((k_scale<uint8_t, uint16_t>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_scale<uint8_t, uint8_t>), grid, block, 0, st, a);
    return hipGetLastError();
}

// deinterlacing source (kernels/deint.h): one workgroup per tile of DI_TW x DI_TH output samples, Y, then Cb, then Cr; the argument block travels by value.
// 10,368 bytes of LDS: four workgroups per CU (4 waves per SIMD) take 41 KB of the CU's 160
template <typename T> __global__ __launch_bounds__(NT, 4) void k_deint(const DeintArgs a)
{
    __shared__ __align__(16) DeintShared s;
    GpuExec ex;
    deint_tile_program<T>(ex, s, a, (int)blockIdx.x);
}
hipError_t launch_deint(hipStream_t st, const DeintArgs &a, bool is16)
{
    const dim3 grid((unsigned)deint_workgroups(a.pw, a.ph)), block(NT);
    if (is16) hipLaunchKernelGGL((k_deint<uint16_t>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_deint<uint8_t>), grid, block, 0, st, a);
    return hipGetLastError();
}

// denoising source (kernels/denoise.h): one workgroup per tile of DN_TW x DN_TH output samples, Y, then Cb, then Cr; the argument block travels by value.
// 29,376 bytes of LDS: four workgroups per CU (4 waves per SIMD, at most 128 VGPRs) take 115 KB of the CU's 160
template <typename T> __global__ __launch_bounds__(NT, 4) void k_denoise(const DenoiseArgs a)
{
    __shared__ __align__(16) DenoiseShared s;
    GpuExec ex;
    denoise_tile_program<T>(ex, s, a, (int)blockIdx.x);
}
hipError_t launch_denoise(hipStream_t st, const DenoiseArgs &a, bool is16)
{
    const dim3 grid((unsigned)deint_workgroups(a.f.pw, a.f.ph)), block(NT);
    if (is16) hipLaunchKernelGGL((k_denoise<uint16_t>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_denoise<uint8_t>), grid, block, 0, st, a);
    return hipGetLastError();
}

// inverse telecine (kernels/fieldmatch.h).  k_fm_metrics: one workgroup per luma tile of FM_TW x FM_TH samples, 28,560 bytes of LDS: four workgroups per CU take
// 112 KB of the CU's 160.  k_fm_fold: one workgroup over their partials.  k_fm_weave: the deinterlacer's tiles, no LDS
template <typename T> __global__ __launch_bounds__(NT, 4) void k_fm_metrics(const FmArgs a)
{
    __shared__ __align__(16) FmShared s;
    GpuExec ex;
    fm_metrics_program<T>(ex, s, a, (int)blockIdx.x);
}
__global__ __launch_bounds__(NT) void k_fm_fold(const unsigned long long *part, int n, unsigned long long *out)
{
    __shared__ __align__(16) FmShared s;
    GpuExec ex;
    fm_fold_program(ex, s, part, n, out);
}
template <typename T> __global__ __launch_bounds__(NT) void k_fm_weave(const DeintArgs a)
{
    GpuExec ex;
    fm_weave_program<T>(ex, a, (int)blockIdx.x);
}
hipError_t launch_fm_metrics(hipStream_t st, const FmArgs &a, unsigned long long *out, bool is16)
{
    const int n = fm_workgroups(a.w, a.h);
    if (is16) hipLaunchKernelGGL((k_fm_metrics<uint16_t>), dim3((unsigned)n), dim3(NT), 0, st, a);
    else hipLaunchKernelGGL((k_fm_metrics<uint8_t>), dim3((unsigned)n), dim3(NT), 0, st, a);
    hipLaunchKernelGGL(k_fm_fold, dim3(1), dim3(NT), 0, st, a.part, n, out);
    return hipGetLastError();
}
hipError_t launch_fm_weave(hipStream_t st, const DeintArgs &a, bool is16)
{
    const dim3 grid((unsigned)deint_workgroups(a.pw, a.ph)), block(NT);
    if (is16) hipLaunchKernelGGL((k_fm_weave<uint16_t>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_fm_weave<uint8_t>), grid, block, 0, st, a);
    return hipGetLastError();
}

// frame-rate multiplication (kernels/mcfi.h).  k_mcfi_search: one workgroup per tile of MC_SB x MC_SB blocks, 37,892 bytes of LDS: four workgroups per CU take
// 148 KB of the CU's 160.  k_mcfi_field: sixteen blocks per workgroup and one more workgroup for the fold of D.  k_mcfi_render: one workgroup per tile of
// MR_TW x MR_TH output samples, Y, then Cb, then Cr, 62,760 bytes of LDS: two workgroups per CU take 123 KB
template <typename T> __global__ __launch_bounds__(NT, 4) void k_mcfi_search(const McfiSearchArgs a)
{
    __shared__ __align__(16) McfiSearchShared s;
    GpuExec ex;
    mcfi_search_program<T>(ex, s, a, (int)blockIdx.x);
}
template <typename T> __global__ __launch_bounds__(NT, 4) void k_mcfi_field(const McfiFieldArgs a)
{
    __shared__ __align__(16) McfiFieldShared s;
    GpuExec ex;
    mcfi_field_program<T>(ex, s, a, (int)blockIdx.x);
}
template <typename T> __global__ __launch_bounds__(NT, 2) void k_mcfi_render(const McfiRenderArgs a)
{
    __shared__ __align__(16) McfiRenderShared s;
    GpuExec ex;
    mcfi_render_program<T>(ex, s, a, (int)blockIdx.x);
}
hipError_t launch_mcfi_search(hipStream_t st, const McfiSearchArgs &a, bool is16)
{
    const dim3 grid((unsigned)mcfi_search_workgroups(a.w, a.h)), block(NT);
    if (is16) hipLaunchKernelGGL((k_mcfi_search<uint16_t>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_mcfi_search<uint8_t>), grid, block, 0, st, a);
    return hipGetLastError();
}
hipError_t launch_mcfi_field(hipStream_t st, const McfiFieldArgs &f, bool is16)
{
    const dim3 grid((unsigned)mcfi_field_workgroups(f.w, f.h)), block(NT);
    if (is16) hipLaunchKernelGGL((k_mcfi_field<uint16_t>), grid, block, 0, st, f);
    else hipLaunchKernelGGL((k_mcfi_field<uint8_t>), grid, block, 0, st, f);
    return hipGetLastError();
}
hipError_t launch_mcfi_vectors(hipStream_t st, const McfiSearchArgs &a, const McfiFieldArgs &f, bool is16)
{
    const hipError_t e = launch_mcfi_search(st, a, is16);
    return e != hipSuccess ? e : launch_mcfi_field(st, f, is16);
}
hipError_t launch_mcfi_render(hipStream_t st, const McfiRenderArgs &a, bool is16)
{
    const dim3 grid((unsigned)mcfi_render_workgroups(a.pw, a.ph)), block(NT);
    if (is16) hipLaunchKernelGGL((k_mcfi_render<uint16_t>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_mcfi_render<uint8_t>), grid, block, 0, st, a);
    return hipGetLastError();
}

// upscaling source (kernels/upscale.h): one workgroup per tile of UP_TW x UP_TH output samples, Y, then Cb, then Cr; the argument block travels by value.
// 15,984 bytes of LDS; the launch bounds ask for eight workgroups per CU (8 waves per SIMD, 64 VGPRs), which the registers allow
template <typename TI, typename TO> __global__ __launch_bounds__(NT, 8) void k_upscale(const UpscaleArgs a)
{
    __shared__ __align__(16) UpscaleShared s;
    GpuExec ex;
    upscale_tile_program<TI, TO>(ex, s, a, (int)blockIdx.x);
}
hipError_t launch_upscale(hipStream_t st, const UpscaleArgs &a, bool in16, bool out16)
{
    const dim3 grid((unsigned)upscale_workgroups(a.pw, a.ph)), block(NT);
    if (in16 && out16) hipLaunchKernelGGL((k_upscale<uint16_t, uint16_t>), grid, block, 0, st, a);
    else if (in16) hipLaunchKernelGGL((k_upscale<uint16_t, uint8_t>), grid, block, 0, st, a);
    else if (out16) hipLaunchKernelGGL((k_upscale<uint8_t, uint16_t>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_upscale<uint8_t, uint8_t>), grid, block, 0, st, a);
    return hipGetLastError();
}

// learned super-resolution (kernels/sr_conv.h): one workgroup per tile of SR_TW x SR_TH output pixels, every output channel of the layer.  Two workgroups per
// CU: the input tile of 192 channels takes 72,000 bytes of LDS
template <int CIN, int NB, bool PLANAR> __global__ __launch_bounds__(NT, SR_PER_CU) void k_sr_conv(const SrConvArgs a)
{
    __shared__ __align__(16) SrShared<CIN> s;
    GpuExec ex;
    sr_conv_program<CIN, NB, PLANAR>(ex, s, a, (int)blockIdx.x);
}
template <typename TI, bool FLT> __global__ __launch_bounds__(NT) void k_sr_input(const SrInputArgs a)
{
    GpuExec ex;
    sr_input_program<TI, FLT>(ex, a, (int)blockIdx.x);
}
hipError_t launch_sr_conv(hipStream_t st, const SrConvArgs &a, int cin, int cout, bool planar)
{
    const dim3 grid((unsigned)sr_conv_workgroups(a.w, a.h)), block(NT);
    if (planar && cin == 64 && cout == 16) hipLaunchKernelGGL((k_sr_conv<64, 1, true>), grid, block, 0, st, a);
    else if (planar) return hipErrorInvalidValue;
    else if (cin == 32 && cout == 64) hipLaunchKernelGGL((k_sr_conv<32, 4, false>), grid, block, 0, st, a);
    else if (cin == 64 && cout == 64) hipLaunchKernelGGL((k_sr_conv<64, 4, false>), grid, block, 0, st, a);
    else if (cin == 192 && cout == 64) hipLaunchKernelGGL((k_sr_conv<192, 4, false>), grid, block, 0, st, a);
    else if (cin == 64 && cout == 32) hipLaunchKernelGGL((k_sr_conv<64, 2, false>), grid, block, 0, st, a);
    else if (cin == 96 && cout == 32) hipLaunchKernelGGL((k_sr_conv<96, 2, false>), grid, block, 0, st, a);
    else if (cin == 128 && cout == 32) hipLaunchKernelGGL((k_sr_conv<128, 2, false>), grid, block, 0, st, a);
    else if (cin == 160 && cout == 32) hipLaunchKernelGGL((k_sr_conv<160, 2, false>), grid, block, 0, st, a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}
hipError_t launch_sr_input(hipStream_t st, const SrInputArgs &a, int sample, int elem_size)
{
    const int f = a.unshuffle ? 2 : 1;
    const dim3 grid((unsigned)sr_input_workgroups(a.sw / f, a.sh / f)), block(NT);
    if (sample == 2) hipLaunchKernelGGL((k_sr_input<uint32_t, true>), grid, block, 0, st, a);
    else if (sample == 1) hipLaunchKernelGGL((k_sr_input<uint16_t, true>), grid, block, 0, st, a);
    else if (elem_size == 2) hipLaunchKernelGGL((k_sr_input<uint16_t, false>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_sr_input<uint8_t, false>), grid, block, 0, st, a);
    return hipGetLastError();
}
hipError_t launch_sr_network(hipStream_t st, const SrNet &net, uint8_t *arena, const uint16_t *wpk, const float *bias, int tw, int th)
{
    hipError_t err = hipSuccess;
    sr_for_each_launch(net, arena, wpk, bias, tw, th, [&](int cin, int cout, bool planar, const SrConvArgs &a) {
        err = launch_sr_conv(st, a, cin, cout, planar);
        return err != hipSuccess;
    });
    return err;
}
// compact super-resolution networks (kernels/sr_compact.h): at most SRC_MAX_WG workgroups, each with the layer's weights in LDS, walk the tiles of SRC_TW x SRC_TH
// pixels.  One workgroup per CU: weights and two tile images take 160,256 bytes of LDS at 64 -> 64
template <int CIN, int NA, int TAIL> __global__ __launch_bounds__(NT, SRC_PER_CU) void k_sr_compact(const SrCompactArgs a)
{
    __shared__ __align__(16) SrCompactShared<CIN, NA> s;
    GpuExec ex;
    sr_compact_program<CIN, NA, TAIL>(ex, s, a, (int)blockIdx.x, (int)gridDim.x);
}
hipError_t launch_sr_compact(hipStream_t st, const SrCompactArgs &a, int cin, int tail)
{
    const dim3 grid((unsigned)sr_compact_workgroups(a.w, a.h)), block(NT);
    if (tail == 4 && cin == 64) hipLaunchKernelGGL((k_sr_compact<64, 3, 4>), grid, block, 0, st, a);
    else if (tail == 2 && cin == 64) hipLaunchKernelGGL((k_sr_compact<64, 1, 2>), grid, block, 0, st, a);
    else if (tail) return hipErrorInvalidValue;
    else if (cin == 32) hipLaunchKernelGGL((k_sr_compact<32, 4, 0>), grid, block, 0, st, a);
    else if (cin == 64) hipLaunchKernelGGL((k_sr_compact<64, 4, 0>), grid, block, 0, st, a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}
hipError_t launch_sr_compact_network(hipStream_t st, const SrCompactNet &net, uint8_t *arena, const uint16_t *wpk, const float *par, int sw, int sh)
{
    hipError_t err = hipSuccess;
    sr_compact_for_each_launch(net, arena, wpk, par, sw, sh, [&](int cin, int tail, const SrCompactArgs &a) {
        err = launch_sr_compact(st, a, cin, tail);
        return err != hipSuccess;
    });
    return err;
}
// a Y'CbCr source in front of the network (kernels/sr_yuv.h): NT blocks of 2 x 2 luma samples per workgroup, one a lane
template <typename TI> __global__ __launch_bounds__(NT) void k_sr_from_yuv(const SrYuvArgs a)
{
    GpuExec ex;
    sr_from_yuv_program<TI>(ex, a, (int)blockIdx.x);
}
hipError_t launch_sr_from_yuv(hipStream_t st, const SrYuvArgs &a, bool in16)
{
    const dim3 grid((unsigned)sr_yuv_workgroups(a.sw, a.sh)), block(NT);
    if (in16) hipLaunchKernelGGL((k_sr_from_yuv<uint16_t>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_sr_from_yuv<uint8_t>), grid, block, 0, st, a);
    return hipGetLastError();
}

// RGB source conversion (kernels/ingest_rgb.h): one workgroup per tile of RGB_TW x RGB_TH source pixels, which writes its luma and both chroma tiles
template <typename TI, bool FLT, typename TO> __global__ __launch_bounds__(NT) void k_ingest_rgb(const IngestRgbArgs a)
{
    GpuExec ex;
    ingest_rgb_tile_program<TI, FLT, TO>(ex, a, (int)blockIdx.x);
}
template <typename TO> static void launch_ingest_rgb_to(hipStream_t st, const IngestRgbArgs &a, int sample, int elem_size)
{
    const dim3 grid((unsigned)ingest_rgb_workgroups(a.pw, a.ph)), block(NT);
    if (sample == 2) hipLaunchKernelGGL((k_ingest_rgb<uint32_t, true, TO>), grid, block, 0, st, a);
    else if (sample == 1) hipLaunchKernelGGL((k_ingest_rgb<uint16_t, true, TO>), grid, block, 0, st, a);
    else if (elem_size == 2) hipLaunchKernelGGL((k_ingest_rgb<uint16_t, false, TO>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_ingest_rgb<uint8_t, false, TO>), grid, block, 0, st, a);
}
hipError_t launch_ingest_rgb(hipStream_t st, const IngestRgbArgs &a, int sample, int elem_size, bool out16)
{
    if (out16) launch_ingest_rgb_to<uint16_t>(st, a, sample, elem_size);
    else launch_ingest_rgb_to<uint8_t>(st, a, sample, elem_size);
    return hipGetLastError();
}

// colour table (kernels/lut3d.h): one workgroup per tile of RGB_TW x RGB_TH source pixels, as k_ingest_rgb.  A lane's block of 16 x 2 pixels keeps
// 128 independent table loads in flight and needs 178 .. 185 registers for them; two workgroups per CU (two waves per SIMD, 256 registers each) is the bound that
// builds without scratch: at three the compiler spills 48 .. 76 bytes per lane, at four over 200
template <typename TI, typename TO> __global__ __launch_bounds__(NT, 2) void k_lut3d(const Lut3dArgs a)
{
    GpuExec ex;
    lut3d_tile_program<TI, TO>(ex, a, (int)blockIdx.x);
}
hipError_t launch_lut3d(hipStream_t st, const Lut3dArgs &a, bool in16, bool out16)
{
    const dim3 grid((unsigned)ingest_rgb_workgroups(a.out.pw, a.out.ph)), block(NT);
    if (in16 && out16) hipLaunchKernelGGL((k_lut3d<uint16_t, uint16_t>), grid, block, 0, st, a);
    else if (in16) hipLaunchKernelGGL((k_lut3d<uint16_t, uint8_t>), grid, block, 0, st, a);
    else if (out16) hipLaunchKernelGGL((k_lut3d<uint8_t, uint16_t>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_lut3d<uint8_t, uint8_t>), grid, block, 0, st, a);
    return hipGetLastError();
}

// scene-cut detector: sum of |a - b| over every 4th sample of every 4th row of the luma planes of pictures blockIdx.y - 1... the pair
// (blockIdx.y, blockIdx.y + 1) -> out[blockIdx.y + 1]; wave reduction by shuffles, one atomic per wave
template <typename T> __global__ __launch_bounds__(256) void k_scene_diff(const ScenePic<T> *pics, unsigned long long *out, int w, int h)
{
    const ScenePic<T> a = pics[blockIdx.y], b = pics[blockIdx.y + 1];
    const int qw = (w + 3) >> 2, nq = qw * ((h + 3) >> 2);
    unsigned acc = 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < nq; i += gridDim.x * 256) {
        const int x = (i % qw) * 4, y = (i / qw) * 4;
        const int d = (int)a.p[(ptrdiff_t)y * a.stride + x] - (int)b.p[(ptrdiff_t)y * b.stride + x];
        acc += (unsigned)(d < 0 ? -d : d);
    }
    unsigned long long v = acc;
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(out + blockIdx.y + 1, v);
}
template <typename T> hipError_t launch_scene_diff(hipStream_t st, const ScenePic<T> *pics, unsigned long long *out, int w, int h, int n)
{
    if (n < 2) return hipSuccess;
    hipLaunchKernelGGL(k_scene_diff<T>, dim3(32, (unsigned)(n - 1)), dim3(256), 0, st, pics, out, w, h);
    return hipGetLastError();
}

// sum of squared error between source and final reconstruction, per plane (encoder PSNR statistics)
template <typename T> __global__ __launch_bounds__(256) void k_frame_sse(const SaoArgs<T> *args)
{
    const SaoArgs<T> &a = args[blockIdx.y];
    // four samples of a row per lane and iteration (coded widths are multiples of 8, chroma of 4): dword / qword loads, one division per quad
    const int ql = (a.w * a.h) >> 2, qc = ql >> 2, nq = ql + 2 * qc;
    unsigned long long acc[3] = {0, 0, 0};
#pragma unroll 4
    for (int i = blockIdx.x * 256 + threadIdx.x; i < nq; i += gridDim.x * 256) {
        const int pl = i < ql ? 0 : i < ql + qc ? 1 : 2, k = pl == 0 ? i : pl == 1 ? i - ql : i - ql - qc, qw = (pl ? a.w >> 1 : a.w) >> 2;
        const int x = (k % qw) * 4, y = k / qw;
        T s4[4], o4[4];
        __builtin_memcpy(s4, a.src[pl].p + (ptrdiff_t)y * a.src[pl].stride + x, sizeof s4);
        __builtin_memcpy(o4, a.out[pl].p + (ptrdiff_t)y * a.out[pl].stride + x, sizeof o4);
        unsigned e = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) { const int d = (int)s4[j] - (int)o4[j]; e += (unsigned)(d * d); }
        acc[pl] += e;
    }
    __shared__ unsigned long long red[3];
    if (threadIdx.x < 3) red[threadIdx.x] = 0;
    __syncthreads();
    for (int pl = 0; pl < 3; pl++) {
        unsigned long long v = acc[pl];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&red[pl], v);
    }
    __syncthreads();
    if (threadIdx.x < 3 && red[threadIdx.x]) atomicAdd(a.sse + threadIdx.x, red[threadIdx.x]);
}

// the per-CTU squared errors the SAO programs left (SaoArgs::sse_ctu) -> the picture's three sums: one workgroup per picture, plain stores
template <typename T> __global__ __launch_bounds__(256) void k_sse_fold(const SaoArgs<T> *args, int n_ctu)
{
    const SaoArgs<T> &a = args[blockIdx.x];
    unsigned long long acc[3] = {0, 0, 0};
    for (int i = (int)threadIdx.x; i < n_ctu; i += 256)
        for (int pl = 0; pl < 3; pl++) acc[pl] += a.sse_ctu[3 * i + pl];
    __shared__ unsigned long long red[3][4];
    for (int pl = 0; pl < 3; pl++) {
        unsigned long long v = acc[pl];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
        if ((threadIdx.x & 63) == 0) red[pl][threadIdx.x >> 6] = v;
    }
    __syncthreads();
    if (threadIdx.x < 3) a.sse[threadIdx.x] = red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
}
template <typename T> hipError_t launch_sse_fold(hipStream_t st, const SaoArgs<T> *d_args, int n_ctu, int batch)
{
    hipLaunchKernelGGL(k_sse_fold<T>, dim3((unsigned)batch), dim3(256), 0, st, d_args, n_ctu);
    return hipGetLastError();
}

// decoded picture hash: the final reconstruction of every picture of the batch as three byte streams (kernels/pichash.h).  Segment partials,
// then one workgroup per (component, picture) folds them in stream order: two launches, no atomics, nothing to zero in front
// component c of the picture (args in global memory: a run-time index costs a load, not a private copy)
template <typename T> __device__ __forceinline__ HashPlane hash_plane_of(const SaoArgs<T> &a, int c)
{
    return HashPlane{(const uint8_t *)a.out[c].p, (long long)a.out[c].stride * (long long)sizeof(T), (c ? a.w >> 1 : a.w) * (int)sizeof(T) / 4, c ? a.h >> 1 : a.h};
}
template <typename T> __global__ __launch_bounds__(NT) void k_pic_hash(const SaoArgs<T> *args, uint32_t *part, int part_words, int kind)
{
    __shared__ PicHashShared s;
    GpuExec ex;
    const SaoArgs<T> &a = args[blockIdx.y];
    int blk = (int)blockIdx.x;
    const int c = hash_locate(hash_blocks(hash_plane_of(a, 0)), hash_blocks(hash_plane_of(a, 1)), blk);
    if (c < 0) return;
    pichash_block_program(ex, s, hash_plane_of(a, c), (int)sizeof(T), kind, blk, part + (size_t)blockIdx.y * part_words + blockIdx.x);
}
template <typename T> __global__ __launch_bounds__(NT) void k_pic_hash_fold(const SaoArgs<T> *args, const uint32_t *part, int part_words, int kind, size_t out_off)
{
    __shared__ PicHashShared s;
    GpuExec ex;
    const SaoArgs<T> &a = args[blockIdx.y];
    const int c = (int)blockIdx.x, first = hash_first_block(hash_blocks(hash_plane_of(a, 0)), hash_blocks(hash_plane_of(a, 1)), c);
    pichash_fold_program(ex, s, hash_plane_of(a, c), kind, part + (size_t)blockIdx.y * part_words + first, (uint32_t *)((uint8_t *)a.sse + out_off) + c);
}
int pic_hash_part_words(int w, int h, int bps)
{
    const HashPlane y{nullptr, 0, w * bps / 4, h}, c{nullptr, 0, (w >> 1) * bps / 4, h >> 1};
    return hash_blocks(y) + 2 * hash_blocks(c);
}
template <typename T> hipError_t launch_pic_hash(hipStream_t st, const SaoArgs<T> *d_args, int w, int h, int batch, int kind, uint32_t *part, size_t out_off)
{
    if (kind != 1 && kind != 2) return hipErrorInvalidValue;
    const int nb = pic_hash_part_words(w, h, (int)sizeof(T));
    hipLaunchKernelGGL(k_pic_hash<T>, dim3((unsigned)nb, (unsigned)batch), dim3(NT), 0, st, d_args, part, nb, kind);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(k_pic_hash_fold<T>, dim3(3, (unsigned)batch), dim3(NT), 0, st, d_args, (const uint32_t *)part, nb, kind, out_off);
    return hipGetLastError();
}

// SSIM of every picture of the batch, source against final reconstruction (kernels/ssim.h): region partials, then one workgroup per (component, picture)
// adds them up: two launches, no atomics, nothing to zero in front
template <typename T> __device__ __forceinline__ SsimPlane<T> ssim_plane_of(const SaoArgs<T> &a, int c)
{
    return SsimPlane<T>{a.src[c].p, a.out[c].p, a.src[c].stride, a.out[c].stride, c ? a.w >> 1 : a.w, c ? a.h >> 1 : a.h};
}
template <typename T> __global__ __launch_bounds__(NT) void k_ssim(const SaoArgs<T> *args, long long *part, int part_words)
{
    __shared__ SsimShared s;
    GpuExec ex;
    const SaoArgs<T> &a = args[blockIdx.y];
    int reg = (int)blockIdx.x;
    const int c = ssim_locate(ssim_regions(a.w, a.h), ssim_regions(a.w >> 1, a.h >> 1), reg);
    if (c < 0) return;
    ssim_region_program<T>(ex, s, ssim_plane_of(a, c), reg, part + (size_t)blockIdx.y * part_words + blockIdx.x);
}
template <typename T> __global__ __launch_bounds__(NT) void k_ssim_fold(const SaoArgs<T> *args, const long long *part, int part_words, size_t out_off)
{
    __shared__ SsimShared s;
    GpuExec ex;
    const SaoArgs<T> &a = args[blockIdx.y];
    const int c = (int)blockIdx.x, nr_y = ssim_regions(a.w, a.h), nr_c = ssim_regions(a.w >> 1, a.h >> 1);
    ssim_fold_program(ex, s, c ? nr_c : nr_y, part + (size_t)blockIdx.y * part_words + ssim_first_region(nr_y, nr_c, c), (long long *)((uint8_t *)a.sse + out_off) + c);
}
int ssim_part_words(int w, int h) { return ssim_regions(w, h) + 2 * ssim_regions(w >> 1, h >> 1); }
template <typename T> hipError_t launch_ssim(hipStream_t st, const SaoArgs<T> *d_args, int w, int h, int batch, long long *part, size_t out_off)
{
    if (w < 16 || h < 16 || (w & 7) || (h & 7) || (out_off & 7)) return hipErrorInvalidValue;
    const int nr = ssim_part_words(w, h);
    hipLaunchKernelGGL(k_ssim<T>, dim3((unsigned)nr, (unsigned)batch), dim3(NT), 0, st, d_args, part, nr);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(k_ssim_fold<T>, dim3(3, (unsigned)batch), dim3(NT), 0, st, d_args, (const long long *)part, nr, out_off);
    return hipGetLastError();
}

// Head of a P step in ONE launch (three tiny kernels before: every launch boundary on the compute stream costs ~6 us, a step had ten): the border pad of
// the picture the previous step finished (only the next picture's searches read the border), the 1/4-size pictures of this step's source and reference,
// and the step's cost parameters.  blockIdx.x selects the job, blockIdx.y the lane.
template <typename T> __global__ __launch_bounds__(256) void k_prep_p_step(const SaoArgs<T> *prev, int n_pad_blocks, const PreArgs<T> *pre, int n_low_blocks,
                                                                           IntraArgs<T> *ia, InterArgs<T> *ea, SaoArgs<T> *sa, StepParams p)
{
    int b = (int)blockIdx.x;
    const int g = (int)blockIdx.y;
    if (b < n_pad_blocks) {
        const SaoArgs<T> &a = prev[g];
        const int ny = pad_border_quads(a.w, a.h, PAD_Y), ncp = pad_border_quads(a.w >> 1, a.h >> 1, PAD_C);
        int i = b * 256 + (int)threadIdx.x;
        if (i < ny) { pad_border_quad<T>(a.out[0], a.w, a.h, PAD_Y, i, a.halo_top, a.halo_bottom); return; }
        i -= ny;
        if (i < ncp) { pad_border_quad<T>(a.out[1], a.w >> 1, a.h >> 1, PAD_C, i, a.halo_top >> 1, a.halo_bottom >> 1); return; }
        i -= ncp;
        if (i < ncp) pad_border_quad<T>(a.out[2], a.w >> 1, a.h >> 1, PAD_C, i, a.halo_top >> 1, a.halo_bottom >> 1);
        return;
    }
    b -= n_pad_blocks;
    if (b < n_low_blocks) { lowres_sample<T>(pre[g], b * 256 + (int)threadIdx.x); return; }
    if (threadIdx.x == 0) {
        CostParams c = p.prm[g];
        ea[g].prm = c; sa[g].prm = c;
        c.tile_cols = p.p_tile_cols; c.tile_rows = p.p_tile_rows;      // P pictures use PPS 0 (one tile, or cfg.p_tiles' grid)
        ia[g].prm = c;
    }
    if (threadIdx.x < 4) sa[g].sse[threadIdx.x] = 0;
}

// ------------------------------------------------------------------------------------------ launchers
template <typename T> hipError_t launch_prep_p_step(hipStream_t st, const SaoArgs<T> *prev, const PreArgs<T> *pre, IntraArgs<T> *ia, InterArgs<T> *ea, SaoArgs<T> *sa,
                                                    const StepParams &p, int w, int h, int batch)
{
    if (batch > MAX_LANES) return hipErrorInvalidValue;
    const int n_pad = prev ? (pad_border_quads(w, h, PAD_Y) + 2 * pad_border_quads(w >> 1, h >> 1, PAD_C) + 255) / 256 : 0;
    const int n_low = pre ? (2 * (w >> 2) * (h >> 2) + 255) / 256 : 0;
    hipLaunchKernelGGL(k_prep_p_step<T>, dim3((unsigned)(n_pad + n_low + 1), (unsigned)batch), dim3(256), 0, st, prev, n_pad, pre, n_low, ia, ea, sa, p);
    return hipGetLastError();
}
template <typename T> hipError_t launch_frame_sse(hipStream_t st, const SaoArgs<T> *d_args, int batch)
{
    hipLaunchKernelGGL(k_frame_sse<T>, dim3(256, (unsigned)batch), dim3(256), 0, st, d_args);      // 3 same-address atomics per block: few, fat blocks
    return hipGetLastError();
}
template <typename K> static hipError_t ensure_smem(K kernel, size_t bytes)
{
    if (bytes <= 48 * 1024) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

template <typename T> hipError_t launch_me_search(hipStream_t st, const InterArgs<T> *d_args, int n_ctu, int batch, int R, int list)
{
    size_t smem = round16(sizeof(MeShared<T>)) + round16((size_t)me_win_elems(R));      // the window holds 8-bit samples for every T
    auto kernel = R == 15 ? k_me_search<T, 15> : k_me_search<T, 0>;
    hipError_t e = ensure_smem(kernel, smem);
    if (e != hipSuccess) return e;
    dim3 grid((unsigned)(((n_ctu + 7) >> 3) << 3), (unsigned)batch);
    hipLaunchKernelGGL(kernel, grid, dim3(NT), smem, st, d_args, n_ctu, list);
    return hipGetLastError();
}

template <typename T> hipError_t launch_inter_ctu(hipStream_t st, const InterArgs<T> *d_args, int n_ctu, int batch, int R)
{
    const InterLds l = inter_lds<T>(R);
    auto kernel = l.y == inter_win_in<T>() ? k_inter_ctu<T, true> : k_inter_ctu<T, false>;
    hipError_t e = ensure_smem(kernel, l.bytes);
    if (e != hipSuccess) return e;
    dim3 grid((unsigned)(((n_ctu + 7) >> 3) << 3), (unsigned)batch);
    hipLaunchKernelGGL(kernel, grid, dim3(NT), l.bytes, st, d_args, n_ctu);
    return hipGetLastError();
}

template <typename T> hipError_t launch_inter_ctu_b(hipStream_t st, const InterArgs<T> *d_args, int n_ctu, int batch, int R)
{
    const size_t smem = inter_b_lds<T>(R).bytes;
    hipError_t e = ensure_smem(k_inter_ctu_b<T>, smem);
    if (e != hipSuccess) return e;
    dim3 grid((unsigned)(((n_ctu + 7) >> 3) << 3), (unsigned)batch);
    hipLaunchKernelGGL(k_inter_ctu_b<T>, grid, dim3(NT), smem, st, d_args, n_ctu);
    return hipGetLastError();
}

// stage A: every CTU of every picture at once (the first launch of launch_intra_picture; alone: mihevc_k_intra_plan)
template <typename T> static hipError_t launch_intra_plan(hipStream_t st, const IntraArgs<T> *d_args, int n_ctu, int batch)
{
    const size_t smem = round16(sizeof(IntraShared<T>));
    hipError_t e = ensure_smem(k_intra_plan<T>, smem);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_intra_plan<T>, dim3((unsigned)(((n_ctu + 7) >> 3) << 3), (unsigned)batch), dim3(NT), smem, st, d_args, n_ctu);
    return hipGetLastError();
}

template <typename T> hipError_t launch_intra_picture(hipStream_t st, const IntraArgs<T> *d_args, int ctus_w, int ctus_h, int batch, int tile_cols, int tile_rows, hipEvent_t after_plan)
{
    size_t smem = round16(sizeof(IntraShared<T>));
    hipError_t e = ensure_smem(k_intra_diag<T>, smem);
    if (e != hipSuccess) return e;
    if (tile_cols < 1) tile_cols = 1;
    if (tile_rows < 1) tile_rows = 1;
    const int n_ctu = ctus_w * ctus_h;
    e = launch_intra_plan<T>(st, d_args, n_ctu, batch);
    if (e != hipSuccess) return e;
    if (after_plan) { e = hipEventRecord(after_plan, st); if (e != hipSuccess) return e; }      // from here on the stream runs the latency-bound anti-diagonal chain
    // stage B, per tile one anti-diagonal at a time; uniform spacing: the widest column / tallest row is ceil(n_ctb / n_tiles)
    const int colw = (ctus_w + tile_cols - 1) / tile_cols, rowh = (ctus_h + tile_rows - 1) / tile_rows;
    for (int d = 0; d <= (colw - 1) + 2 * (rowh - 1); d++)
        hipLaunchKernelGGL(k_intra_diag<T>, dim3((unsigned)(tile_cols * tile_rows * rowh), (unsigned)batch), dim3(NT), smem, st, d_args, d, rowh);
    return hipGetLastError();
}

template <typename T> hipError_t launch_pre_search(hipStream_t st, const PreArgs<T> *d_args, int w, int h, int n_ctu, int batch, bool with_lowres)
{
    const int n = 2 * (w >> 2) * (h >> 2);
    if (with_lowres) hipLaunchKernelGGL(k_lowres<T>, dim3((unsigned)((n + 255) / 256), (unsigned)batch), dim3(256), 0, st, d_args);      // else: k_prep_p_step made the pictures
    hipLaunchKernelGGL(k_pre_search<T>, dim3((unsigned)n_ctu, (unsigned)batch), dim3(NT), 0, st, d_args, n_ctu);
    return hipGetLastError();
}

// every picture of a chunk at once (args[i]: picture i in stream order): 1/4-size pictures of the SOURCES, then the search centres of picture i from
// lsrc (its own) against lref (its predecessor's) — PreArgs::ref is not read
template <typename T> __global__ __launch_bounds__(256) void k_lowres_src(const PreArgs<T> *args)
{
    const PreArgs<T> &a = args[blockIdx.y];
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i < (a.w >> 2) * (a.h >> 2)) lowres_sample<T>(a, i);
}
template <typename T> hipError_t launch_pre_search_chunk(hipStream_t st, const PreArgs<T> *d_args, int w, int h, int n_ctu, int n_pictures)
{
    if (n_pictures <= 0) return hipSuccess;
    const int n = (w >> 2) * (h >> 2);
    hipLaunchKernelGGL(k_lowres_src<T>, dim3((unsigned)((n + 255) / 256), (unsigned)n_pictures), dim3(256), 0, st, d_args);
    hipLaunchKernelGGL(k_pre_search<T>, dim3((unsigned)n_ctu, (unsigned)n_pictures), dim3(NT), 0, st, d_args, n_ctu);
    return hipGetLastError();
}

template <typename T> hipError_t launch_intra_p(hipStream_t st, const IntraArgs<T> *d_args, int n_ctu, int batch)
{
    size_t smem = round16(sizeof(IntraShared<T>));
    hipError_t e = ensure_smem(k_intra_p<T>, smem);
    if (e != hipSuccess) return e;
    for (int round = 0; round < 2; round++)
        hipLaunchKernelGGL(k_intra_p<T>, dim3((unsigned)n_ctu, (unsigned)batch), dim3(NT), smem, st, d_args, n_ctu, round);
    return hipGetLastError();
}

template <typename T> hipError_t launch_deblock(hipStream_t st, const DeblockArgs<T> *d_v, const DeblockArgs<T> *d_h, int w, int h, int batch)
{
    int segs = (w >> 3) * (h >> 3) * 2;
    dim3 grid((unsigned)((segs + 255) / 256), (unsigned)batch);
    hipLaunchKernelGGL(k_deblock<T>, grid, dim3(256), 0, st, d_v);
    hipLaunchKernelGGL(k_deblock<T>, grid, dim3(256), 0, st, d_h);
    return hipGetLastError();
}

template <typename T> hipError_t launch_sao(hipStream_t st, const SaoArgs<T> *d_args, int w, int h, int batch, bool decide)
{
    int n_ctu = ((w + CTU - 1) / CTU) * ((h + CTU - 1) / CTU);
    if (decide) {        // the CTU program decides AND applies (its deblocked tile is in LDS): no second pass
        hipLaunchKernelGGL(k_sao_decide<T>, dim3((unsigned)(((n_ctu + 7) >> 3) << 3), (unsigned)batch), dim3(NT), 0, st, d_args, n_ctu);
        return hipGetLastError();
    }
    int n = (w * h + (w * h >> 1)) >> 2;
    hipLaunchKernelGGL(k_sao_apply<T>, dim3((unsigned)((n + 255) / 256), (unsigned)batch), dim3(256), 0, st, d_args);
    return hipGetLastError();
}

template <typename T> hipError_t launch_pad(hipStream_t st, const SaoArgs<T> *d_args, int w, int h, int batch)
{
    int n = pad_border_quads(w, h, PAD_Y) + 2 * pad_border_quads(w >> 1, h >> 1, PAD_C);
    hipLaunchKernelGGL(k_pad<T>, dim3((unsigned)((n + 255) / 256), (unsigned)batch), dim3(256), 0, st, d_args);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void k_copy_rows(const RowCopy *jobs)
{
    copy_rows_item(jobs[blockIdx.y], (int)(blockIdx.x * 256 + threadIdx.x), (int)(gridDim.x * 256));
}
hipError_t launch_copy_rows(hipStream_t st, const RowCopy *d_jobs, int n_jobs, int blocks_per_job)
{
    if (n_jobs <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_copy_rows, dim3((unsigned)blocks_per_job, (unsigned)n_jobs), dim3(256), 0, st, d_jobs);
    return hipGetLastError();
}

template <typename T> hipError_t alloc_plane(DevPlane<T> &d, int w, int h, int pad)
{
    d.w = w; d.h = h; d.pad = pad;
    d.pl.stride = (w + 2 * pad + 63) & ~63;
    hipError_t e = hipMalloc((void **)&d.base, (size_t)d.pl.stride * (h + 2 * pad) * sizeof(T));
    if (e != hipSuccess) { d.base = nullptr; return e; }
    d.pl.p = d.base + (size_t)pad * d.pl.stride + pad;
    return hipSuccess;
}
template <typename T> void free_plane(DevPlane<T> &d)
{
    if (d.base) (void)hipFree(d.base);
    d.base = nullptr; d.pl.p = nullptr;
}

int gfx950_device_count()
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    int ok = 0;
    for (int i = 0; i < n; i++) {
        hipDeviceProp_t p;
        if (hipGetDeviceProperties(&p, i) == hipSuccess && strncmp(p.gcnArchName, "gfx950", 6) == 0) ok++;
    }
    return ok;
}

#define INSTANTIATE(T)                                                                                                   \
    template hipError_t launch_me_search<T>(hipStream_t, const InterArgs<T> *, int, int, int, int);                     \
    template hipError_t launch_inter_ctu_b<T>(hipStream_t, const InterArgs<T> *, int, int, int);                        \
    template hipError_t launch_inter_ctu<T>(hipStream_t, const InterArgs<T> *, int, int, int);                          \
    template hipError_t launch_intra_picture<T>(hipStream_t, const IntraArgs<T> *, int, int, int, int, int, hipEvent_t);    \
    template hipError_t launch_intra_p<T>(hipStream_t, const IntraArgs<T> *, int, int);                                       \
    template hipError_t launch_pre_search<T>(hipStream_t, const PreArgs<T> *, int, int, int, int, bool);                \
    template hipError_t launch_pre_search_chunk<T>(hipStream_t, const PreArgs<T> *, int, int, int, int);                \
    template hipError_t launch_prep_p_step<T>(hipStream_t, const SaoArgs<T> *, const PreArgs<T> *, IntraArgs<T> *, InterArgs<T> *, SaoArgs<T> *, const StepParams &, int, int, int); \
    template hipError_t launch_deblock<T>(hipStream_t, const DeblockArgs<T> *, const DeblockArgs<T> *, int, int, int);  \
    template hipError_t launch_sao<T>(hipStream_t, const SaoArgs<T> *, int, int, int, bool);                            \
    template hipError_t launch_pad<T>(hipStream_t, const SaoArgs<T> *, int, int, int);                                  \
    template hipError_t launch_frame_sse<T>(hipStream_t, const SaoArgs<T> *, int);                                       \
    template hipError_t launch_sse_fold<T>(hipStream_t, const SaoArgs<T> *, int, int);                                   \
    template hipError_t launch_pic_hash<T>(hipStream_t, const SaoArgs<T> *, int, int, int, int, uint32_t *, size_t);           \
    template hipError_t launch_ssim<T>(hipStream_t, const SaoArgs<T> *, int, int, int, long long *, size_t);                   \
    template hipError_t launch_extend_margin<T>(hipStream_t, Plane<T>, int, int, int, int);                             \
    template hipError_t launch_scene_diff<T>(hipStream_t, const ScenePic<T> *, unsigned long long *, int, int, int);            \
    template hipError_t alloc_plane<T>(DevPlane<T> &, int, int, int);                                                   \
    template void free_plane<T>(DevPlane<T> &);
INSTANTIATE(uint8_t)
INSTANTIATE(uint16_t)

// ------------------------------------------------------------------------------------------ K3 alone (parity/bench entry)
// One workgroup per batch of residual blocks laid out as a pseudo-CTU: the blocks of one launch share log2n.  sign_hide: with sign data
// hiding, every block's groups in the 4x4 scan `scan` (residual_pipeline)
__global__ __launch_bounds__(NT) void k_transform_blocks(const int16_t *res, int16_t *lvl, int16_t *rec, int n_blocks, int log2n, int qp,
                                                         int bit_depth, int intra, int scan, int sign_hide)
{
    __shared__ ResidualShared s;
    GpuExec ex;
    const int n = 1 << log2n, per = 1024 >> (2 * log2n);          // luma-area blocks per workgroup
    const int first = blockIdx.x * per;
    residual_init(ex, s);
    ex.phase([&](int tid) {
        if (tid < 16) {
            int tx = (tid & 3) * 8, ty = (tid >> 2) * 8;
            int blk = first + (ty >> (log2n < 3 ? 3 : log2n)) * (32 >> (log2n < 3 ? 3 : log2n)) + (tx >> (log2n < 3 ? 3 : log2n));
            s.tu_log2[tid] = (log2n >= 3 && blk < n_blocks) ? (uint8_t)log2n : 0;
            s.tu_intra[tid] = (uint8_t)intra;
        }
        for (int i = tid; i < 1536; i += NT) s.res[i] = 0;
    });
    ex.phase([&](int tid) {
        for (int i = tid; i < 1024; i += NT) {
            int x = i & 31, y = i >> 5, blk = first + (y >> log2n) * (32 >> log2n) + (x >> log2n);
            if (blk < n_blocks) s.res[i] = res[(size_t)blk * n * n + (y & (n - 1)) * n + (x & (n - 1))];
        }
        fill_desc(s, whole_ctu(), tid, [&](const SampleLoc &) { return scan; });
    });
    residual_pipeline(ex, s, qp, qp, bit_depth, whole_ctu(), 0, sign_hide);
    ex.phase([&](int tid) {
        for (int i = tid; i < 1024; i += NT) {
            int x = i & 31, y = i >> 5, blk = first + (y >> log2n) * (32 >> log2n) + (x >> log2n);
            if (blk >= n_blocks) continue;
            size_t o = (size_t)blk * n * n + (y & (n - 1)) * n + (x & (n - 1));
            lvl[o] = s.lvl[i];
            rec[o] = s.res[i];
        }
    });
}

// 4x4 TUs (DCT, or DST-VII for intra luma): 16 lanes per block, NT / 16 blocks per workgroup (transform4_program on the 4x4 core of residual.h)
__global__ __launch_bounds__(NT) void k_transform4_blocks(const int16_t *res, int16_t *lvl, int16_t *rec, int n_blocks, int qp, int bit_depth, int intra, int dst,
                                                          int scan, int sign_hide)
{
    __shared__ Transform4Shared s;
    GpuExec ex;
    transform4_program(ex, s, res, lvl, rec, n_blocks, (int)blockIdx.x * (NT / 16), qp, bit_depth, intra, dst, scan, sign_hide);
}

}  // namespace mihevc

// ================================================================================================ C ABI: stages
using namespace mihevc;

namespace {

struct DevBuf {      // RAII device allocation
    void *p = nullptr;
    hipError_t alloc(size_t n) { return hipMalloc(&p, n ? n : 1); }
    ~DevBuf() { if (p) (void)hipFree(p); }
    template <typename U> U *as() const { return static_cast<U *>(p); }
};
#define CK(expr)                                     \
    do {                                             \
        hipError_t e_ = (expr);                      \
        if (e_ != hipSuccess) return MIHEVC_EDEVICE; \
    } while (0)

// n host blocks of A into a new device buffer
template <typename A> int to_device(DevBuf &d, const A *h, size_t n = 1)
{
    CK(d.alloc(n * sizeof(A)));
    CK(hipMemcpy(d.p, h, n * sizeof(A), hipMemcpyHostToDevice));
    return 0;
}

template <typename T> struct Planes3 {
    DevPlane<T> p[3];
    Plane<T> rw[3]{};            // views for the argument builders (stage_args.h)
    Plane<const T> ro[3]{};
    int alloc(int w, int h, bool padded)
    {
        for (int i = 0; i < 3; i++) {
            if (alloc_plane<T>(p[i], i ? w / 2 : w, i ? h / 2 : h, padded ? (i ? PAD_C : PAD_Y) : 0) != hipSuccess) return MIHEVC_ENOMEM;
            rw[i] = p[i].pl; ro[i] = {p[i].pl.p, p[i].pl.stride};
        }
        return 0;
    }
    int upload(const void *const *src)
    {
        for (int i = 0; i < 3; i++)
            CK(hipMemcpy2D(p[i].pl.p, p[i].pl.stride * sizeof(T), src[i], p[i].w * sizeof(T), p[i].w * sizeof(T), p[i].h, hipMemcpyHostToDevice));
        return 0;
    }
    int download(void *const *dst)
    {
        for (int i = 0; i < 3; i++)
            CK(hipMemcpy2D(dst[i], p[i].w * sizeof(T), p[i].pl.p, p[i].pl.stride * sizeof(T), p[i].w * sizeof(T), p[i].h, hipMemcpyDeviceToHost));
        return 0;
    }
    ~Planes3() { for (auto &x : p) free_plane<T>(x); }
};

struct DevAnalysis {     // what an analysis stage writes: CU records (zeroed), levels, rate estimate (zeroed)
    DevBuf cu, coef[3], est;
    size_t n8 = 0, ny = 0;
    int alloc(int w, int h)
    {
        n8 = (size_t)(w / 8) * (h / 8); ny = (size_t)w * h;
        CK(cu.alloc(n8 * sizeof(mihevc_cu_rec))); CK(coef[0].alloc(ny * 2)); CK(coef[1].alloc(ny / 2)); CK(coef[2].alloc(ny / 2)); CK(est.alloc(8));
        CK(hipMemset(cu.p, 0, n8 * sizeof(mihevc_cu_rec))); CK(hipMemset(est.p, 0, 8));
        return 0;
    }
    AnalysisOut view() const { return AnalysisOut{cu.as<mihevc_cu_rec>(), {coef[0].as<int16_t>(), coef[1].as<int16_t>(), coef[2].as<int16_t>()}, est.as<unsigned long long>()}; }
    int download(mihevc_cu_rec *hcu, int16_t *const *hcoef, uint64_t *hest) const
    {
        CK(hipMemcpy(hcu, cu.p, n8 * sizeof(mihevc_cu_rec), hipMemcpyDeviceToHost));
        for (int i = 0; i < 3; i++) CK(hipMemcpy(hcoef[i], coef[i].p, i ? ny / 2 : ny * 2, hipMemcpyDeviceToHost));
        if (hest) CK(hipMemcpy(hest, est.p, 8, hipMemcpyDeviceToHost));
        return 0;
    }
};

bool geometry_ok(int w, int h) { return w >= 16 && h >= 16 && !(w & 7) && !(h & 7) && w <= 8192 && h <= 4352; }

// s, r, coef: the three planes (Y, Cb, Cr) of the source, the reconstruction, the levels
template <typename T>
int stage_intra(const void *const *s, int w, int h, const mihevc_cost_params *prm, void *const *r, mihevc_cu_rec *cu, int16_t *const *coef, uint64_t *est)
{
    Planes3<T> src, rec;
    if (src.alloc(w, h, false) || rec.alloc(w, h, false)) return MIHEVC_ENOMEM;
    if (int e = src.upload(s)) return e;
    DevAnalysis out;
    DevBuf dplan, dargs;
    if (int e = out.alloc(w, h)) return e;
    CK(dplan.alloc((size_t)ctus_of(w) * ctus_of(h) * sizeof(IntraPlan)));
    const IntraArgs<T> a = intra_args<T>(src.ro, rec.rw, w, h, cost_params_of(*prm), out.view(), dplan.as<IntraPlan>());
    if (int e = to_device(dargs, &a)) return e;
    CK(launch_intra_picture<T>(0, dargs.as<IntraArgs<T>>(), a.ctus_w, a.ctus_h, 1, a.prm.tile_cols, a.prm.tile_rows, nullptr));
    CK(hipDeviceSynchronize());
    if (int e = rec.download(r)) return e;
    return out.download(cu, coef, est);
}

// the plan of every CTU as k_intra_plan leaves it for the code stage (IntraArgs::plan); bytes the kernel never writes (mode / cmode of nodes outside the
// picture, pad) come back as 0
static_assert(sizeof(IntraPlan) == sizeof(mihevc_intra_plan) && sizeof(IntraPlan) == 64, "mihevc_intra_plan is IntraPlan");
template <typename T> int stage_intra_plan(const void *const *s, int w, int h, const mihevc_cost_params *prm, mihevc_intra_plan *plan)
{
    Planes3<T> src;
    if (src.alloc(w, h, false)) return MIHEVC_ENOMEM;
    if (int e = src.upload(s)) return e;
    const size_t n_ctu = (size_t)ctus_of(w) * ctus_of(h);
    DevBuf dplan, dargs;
    CK(dplan.alloc(n_ctu * sizeof(IntraPlan)));
    const Plane<T> none[3]{};       // the plan stage reads the source only
    const IntraArgs<T> a = intra_args<T>(src.ro, none, w, h, cost_params_of(*prm), AnalysisOut{nullptr, {nullptr, nullptr, nullptr}, nullptr}, dplan.as<IntraPlan>());
    if (int e = to_device(dargs, &a)) return e;
    CK(launch_intra_plan<T>(0, dargs.as<IntraArgs<T>>(), (int)n_ctu, 1));
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(plan, dplan.p, n_ctu * sizeof(IntraPlan), hipMemcpyDeviceToHost));
    intra_plan_clear_unwritten(plan, w, h);
    return 0;
}

// A P picture (f1 == nullptr) against the reference f0: border pad, search centres from the 1/4-size pictures (prm->pre_search without centres0),
// the list-0 search, the P CTU program, the intra second pass (prm->intra_in_p).  A B picture between the anchors f0 (list 0) and f1 (list 1):
// border pad of both, the list-0 and list-1 searches, the B CTU program.  centers*, me_dump*: per list, optional
template <typename T>
int stage_inter(const void *const *s, const void *const *f0, const void *const *f1, int w, int h, const mihevc_cost_params *prm, const int16_t *centers0,
                const int16_t *centers1, void *const *r, mihevc_cu_rec *cu, int16_t *const *coef, int32_t *me_dump0, int32_t *me_dump1, uint64_t *est)
{
    const bool b = f1 != nullptr;
    const int nref = b ? 2 : 1;
    Planes3<T> src, ref[2], rec;
    if (src.alloc(w, h, false) || ref[0].alloc(w, h, true) || (b && ref[1].alloc(w, h, true)) || rec.alloc(w, h, false)) return MIHEVC_ENOMEM;
    if (int e = src.upload(s)) return e;
    const void *const *f[2] = {f0, f1};
    const int16_t *centers[2] = {centers0, centers1};
    int32_t *me_dump[2] = {me_dump0, me_dump1};
    for (int l = 0; l < nref; l++)
        if (int e = ref[l].upload(f[l])) return e;
    const CostParams p = cost_params_of(*prm);
    const int n_ctu = ctus_of(w) * ctus_of(h);
    const size_t me_bytes = (size_t)n_ctu * 63 * 4;
    const bool pre = !b && p.pre_search && !centers0;
    DevAnalysis out;
    DevBuf dme[2], dcen[2], dip, dpad, dls, dlr, dpre, dargs, diargs;
    if (int e = out.alloc(w, h)) return e;
    for (int l = 0; l < nref; l++) {
        CK(dme[l].alloc(me_bytes)); CK(dcen[l].alloc((size_t)n_ctu * 4));
        if (centers[l]) CK(hipMemcpy(dcen[l].p, centers[l], (size_t)n_ctu * 4, hipMemcpyHostToDevice));
    }
    // border extension of the uploaded references
    const SaoArgs<T> pa[2] = {picture_args<T>(ref[0].rw, w, h), picture_args<T>(ref[1].rw, w, h)};
    if (int e = to_device(dpad, pa, nref)) return e;
    CK(launch_pad<T>(0, dpad.as<SaoArgs<T>>(), w, h, nref));
    if (!b && p.intra_in_p) { CK(dip.alloc((size_t)n_ctu * sizeof(IpInfo))); CK(hipMemset(dip.p, 0, (size_t)n_ctu * sizeof(IpInfo))); }
    const InterArgs<T> a = inter_args<T>(src.ro, ref[0].ro, b ? ref[1].ro : nullptr, rec.rw, w, h, p, out.view(), centers0 || pre ? dcen[0].as<int16_t>() : nullptr,
                                         centers1 ? dcen[1].as<int16_t>() : nullptr, dme[0].as<int32_t>(), dme[1].as<int32_t>(), dip.as<IpInfo>());
    if (pre) {       // search centres from the 1/4-size pictures
        const size_t ln = (size_t)(w >> 2) * (h >> 2);
        CK(dls.alloc(ln)); CK(dlr.alloc(ln));
        const PreArgs<T> pre_a = pre_args<T>(a, dls.as<uint8_t>(), dlr.as<uint8_t>(), dcen[0].as<int16_t>());
        if (int e = to_device(dpre, &pre_a)) return e;
        CK(launch_pre_search<T>(0, dpre.as<PreArgs<T>>(), w, h, n_ctu, 1, true));
    }
    if (int e = to_device(dargs, &a)) return e;
    CK(launch_me_search<T>(0, dargs.as<InterArgs<T>>(), n_ctu, 1, p.me_range, 0));
    if (b) {
        CK(launch_me_search<T>(0, dargs.as<InterArgs<T>>(), n_ctu, 1, p.me_range, 1));
        CK(launch_inter_ctu_b<T>(0, dargs.as<InterArgs<T>>(), n_ctu, 1, p.me_range));
    } else
        CK(launch_inter_ctu<T>(0, dargs.as<InterArgs<T>>(), n_ctu, 1, p.me_range));
    if (a.ip) {       // intra second pass on the same reconstruction / records / levels
        const IntraArgs<T> ia = intra_in_p_args(a);
        if (int e = to_device(diargs, &ia)) return e;
        CK(launch_intra_p<T>(0, diargs.as<IntraArgs<T>>(), n_ctu, 1));
    }
    CK(hipDeviceSynchronize());
    if (int e = rec.download(r)) return e;
    for (int l = 0; l < nref; l++)
        if (me_dump[l]) CK(hipMemcpy(me_dump[l], dme[l].p, me_bytes, hipMemcpyDeviceToHost));
    return out.download(cu, coef, est);
}

template <typename T> int stage_deblock(void *const *r, int w, int h, const mihevc_cu_rec *cu, int bit_depth)
{
    Planes3<T> rec;
    if (rec.alloc(w, h, false)) return MIHEVC_ENOMEM;
    if (int e = rec.upload(r)) return e;
    DevBuf dcu, dargs;
    if (int e = to_device(dcu, cu, (size_t)(w / 8) * (h / 8))) return e;
    const DeblockArgs<T> a[2] = {deblock_args<T>(rec.rw, w, h, dcu.as<mihevc_cu_rec>(), bit_depth, 0), deblock_args<T>(rec.rw, w, h, dcu.as<mihevc_cu_rec>(), bit_depth, 1)};
    if (int e = to_device(dargs, a, 2)) return e;
    CK(launch_deblock<T>(0, dargs.as<DeblockArgs<T>>(), dargs.as<DeblockArgs<T>>() + 1, w, h, 1));
    CK(hipDeviceSynchronize());
    return rec.download(r);
}

// cu: the fused loop filter, `d` is then the pre-deblock reconstruction
template <typename T>
int stage_sao(const void *const *s, const void *const *d, int w, int h, const mihevc_cost_params *prm, void *const *o, mihevc_sao_ctu *sao, const mihevc_cu_rec *cu = nullptr)
{
    Planes3<T> src, dbk, out;
    if (src.alloc(w, h, false) || dbk.alloc(w, h, false) || out.alloc(w, h, true)) return MIHEVC_ENOMEM;
    if (int e = src.upload(s)) return e;
    if (int e = dbk.upload(d)) return e;
    const int n_ctu = ctus_of(w) * ctus_of(h);
    DevBuf dsao, dargs, dcu;
    CK(dsao.alloc((size_t)n_ctu * sizeof(mihevc_sao_ctu)));
    if (cu) {
        if (int e = to_device(dcu, cu, (size_t)(w / 8) * (h / 8))) return e;
    }
    const SaoArgs<T> a = sao_args<T>(src.ro, dbk.ro, out.rw, w, h, cost_params_of(*prm), dsao.as<mihevc_sao_ctu>(), dcu.as<mihevc_cu_rec>());
    if (int e = to_device(dargs, &a)) return e;
    CK(launch_sao<T>(0, dargs.as<SaoArgs<T>>(), w, h, 1, true));
    CK(launch_pad<T>(0, dargs.as<SaoArgs<T>>(), w, h, 1));
    CK(hipDeviceSynchronize());
    if (int e = out.download(o)) return e;
    CK(hipMemcpy(sao, dsao.p, (size_t)n_ctu * sizeof(mihevc_sao_ctu), hipMemcpyDeviceToHost));
    return MIHEVC_OK;
}

// the decoded picture hash kernels alone, on reference-layout planes (the border of a session's final reconstruction around them)
template <typename T> int stage_picture_hash(const void *const *s, int w, int h, int kind, uint32_t *out)
{
    Planes3<T> pic;
    if (pic.alloc(w, h, true)) return MIHEVC_ENOMEM;
    if (int e = pic.upload(s)) return e;
    DevBuf dargs, dpart, dout;
    CK(dpart.alloc((size_t)pic_hash_part_words(w, h, (int)sizeof(T)) * 4)); CK(dout.alloc(3 * sizeof(uint32_t)));
    const SaoArgs<T> a = picture_args<T>(pic.rw, w, h, dout.as<unsigned long long>());
    if (int e = to_device(dargs, &a)) return e;
    CK(launch_pic_hash<T>(0, dargs.as<SaoArgs<T>>(), w, h, 1, kind, dpart.as<uint32_t>(), 0));
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(out, dout.p, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return MIHEVC_OK;
}

// the SSIM kernels alone: a = source (a plain plane), b = reconstruction (reference layout: in its border), as in a session
template <typename T> int stage_ssim(const void *const *a, const void *const *b, int w, int h, int64_t *sum)
{
    Planes3<T> src, rec;
    if (src.alloc(w, h, false) || rec.alloc(w, h, true)) return MIHEVC_ENOMEM;
    if (int e = src.upload(a)) return e;
    if (int e = rec.upload(b)) return e;
    DevBuf dargs, dpart, dout;
    CK(dargs.alloc(sizeof(SaoArgs<T>))); CK(dpart.alloc((size_t)ssim_part_words(w, h) * sizeof(long long))); CK(dout.alloc(3 * sizeof(long long)));
    SaoArgs<T> sa{};
    for (int i = 0; i < 3; i++) { sa.src[i] = src.ro[i]; sa.out[i] = rec.rw[i]; }
    sa.w = w; sa.h = h; sa.sse = dout.as<unsigned long long>();
    CK(hipMemcpy(dargs.p, &sa, sizeof sa, hipMemcpyHostToDevice));
    CK(launch_ssim<T>(0, dargs.as<SaoArgs<T>>(), w, h, 1, dpart.as<long long>(), 0));
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(sum, dout.p, 3 * sizeof(long long), hipMemcpyDeviceToHost));
    return MIHEVC_OK;
}

// A source plane of a converter as the caller laid it out: the device copy keeps the pitch and starts at the same offset from a 16-byte boundary, so its
// alignment class is the caller's, and it ends with the last sample of the last row.  row, pitch: in elements of es bytes; p becomes the device copy
int upload_as_laid_out(DevBuf &d, const void *&p, int row, int rows, int pitch, size_t es)
{
    const size_t off = (size_t)(uintptr_t)p & 15, bytes = ((size_t)pitch * (rows - 1) + row) * es;
    CK(d.alloc(off + bytes));
    CK(hipMemcpy(d.as<uint8_t>() + off, p, bytes, hipMemcpyHostToDevice));
    p = d.as<uint8_t>() + off;
    return MIHEVC_OK;
}
// the three planes of a planar 4:2:0 frame `in` of w x h, each as the caller laid it out; d: their device copies
int upload_yuv420(DevBuf din[3], const void *d[3], const void *const *in, int w, int h, int pitch_y, int pitch_c, size_t es)
{
    for (int c = 0; c < 3; c++) {
        d[c] = in[c];
        if (int e = upload_as_laid_out(din[c], d[c], c ? w / 2 : w, c ? h / 2 : h, c ? pitch_c : pitch_y, es)) return e;
    }
    return MIHEVC_OK;
}
// the output of a converter: planes of the coded size (the display size rounded up to 8) and of 16-byte aligned stride
template <typename TO> struct ConvertOut {
    Planes3<TO> planes;
    int w, h, stride[3];
    void *p[3];
    int alloc(int sw, int sh)
    {
        w = (sw + 7) & ~7; h = (sh + 7) & ~7;
        if (planes.alloc(w, h, false)) return MIHEVC_ENOMEM;
        for (int c = 0; c < 3; c++) { p[c] = planes.p[c].pl.p; stride[c] = planes.p[c].pl.stride; }
        return MIHEVC_OK;
    }
};
// the scene-cut sums of n consecutive pictures as a session takes them: launch_scene_diff on zeroed sums; the planes keep the pitches they come with
template <typename T> int stage_scene_diff(const void *const *luma, const int32_t *pitch, int n, int w, int h, uint64_t *out)
{
    std::vector<DevBuf> planes((size_t)n);
    std::vector<ScenePic<T>> pics((size_t)n);
    for (int i = 0; i < n; i++) {
        const size_t bytes = (size_t)pitch[i] * h * sizeof(T);
        CK(planes[(size_t)i].alloc(bytes));
        CK(hipMemcpy(planes[(size_t)i].p, luma[i], bytes, hipMemcpyHostToDevice));
        pics[(size_t)i] = ScenePic<T>{planes[(size_t)i].template as<const T>(), pitch[i]};
    }
    DevBuf dpics, dout;
    if (int e = to_device(dpics, pics.data(), (size_t)n)) return e;
    CK(dout.alloc((size_t)n * sizeof(unsigned long long)));
    CK(hipMemset(dout.p, 0, (size_t)n * sizeof(unsigned long long)));
    CK(launch_scene_diff<T>(0, dpics.as<const ScenePic<T>>(), dout.as<unsigned long long>(), w, h, n));
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(out, dout.p, (size_t)n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return MIHEVC_OK;
}

bool convert_geometry_ok(int w, int h, int out_depth)
{
    return w >= 16 && h >= 16 && !(w & 1) && !(h & 1) && w <= 8192 && h <= 4352 && (out_depth == 8 || out_depth == 10);
}

// the conversion kernel alone
template <typename TO>
int stage_convert(const mihevc_src_format &f, const void *const *src, int w, int h, int pitch_y, int pitch_c, int out_depth, void *const *out)
{
    const size_t es = f.bit_depth > 8 ? 2 : 1;
    DevBuf din[3];
    ConvertOut<TO> dst;
    if (int e = dst.alloc(w, h)) return e;
    const void *dsrc[3] = {src[0], src[1], f.semi_planar ? nullptr : src[2]};
    for (int c = 0; c < (f.semi_planar ? 2 : 3); c++)
        if (int e = upload_as_laid_out(din[c], dsrc[c], c ? src_chroma_row(f, w) : w, c ? src_chroma_rows(f, h) : h, c ? pitch_c : pitch_y, es)) return e;
    const IngestArgs a = ingest_args(f, dsrc[0], dsrc[1], dsrc[2], pitch_y, pitch_c, w, h, dst.w, dst.h, out_depth, dst.p, dst.stride);
    CK(launch_ingest(0, a, es == 2, sizeof(TO) == 2));
    CK(hipDeviceSynchronize());
    return dst.planes.download(out);
}

// the RGB conversion kernel alone
template <typename TO>
int stage_convert_rgb(const mihevc_rgb_format &f, const void *const *src, int w, int h, int pitch, int out_depth, void *const *out)
{
    const size_t es = (size_t)rgb_elem_size(f);
    DevBuf din[3];
    ConvertOut<TO> dst;
    if (int e = dst.alloc(w, h)) return e;
    const void *dsrc[3] = {src[0], src[1], src[2]};
    for (int c = 0; c < rgb_planes(f); c++)
        if (int e = upload_as_laid_out(din[c], dsrc[c], rgb_row_elems(f, w), h, pitch, es)) return e;
    const IngestRgbArgs a = ingest_rgb_args(f, f.matrix, f.range == 2, dsrc[0], dsrc[1], dsrc[2], pitch, w, h, dst.w, dst.h, out_depth, dst.p, dst.stride);
    CK(launch_ingest_rgb(0, a, f.sample, (int)es, sizeof(TO) == 2));
    CK(hipDeviceSynchronize());
    return dst.planes.download(out);
}

// the colour table kernel alone; out: the caller's planes with their own strides
template <typename TO>
int stage_lut3d(const mihevc_lut3d_src &f, int n, const uint16_t *table, const void *const *src, int w, int h, int pitch_y, int pitch_c, int out_depth, int out_matrix,
                bool out_full, void *const *out, const int *out_stride)
{
    const size_t es = f.bit_depth > 8 ? 2 : 1, entries = (size_t)n * n * n;
    DevBuf din[3], dtab;
    ConvertOut<TO> dst;
    if (int e = dst.alloc(w, h)) return e;
    const void *dsrc[3];
    if (int e = upload_yuv420(din, dsrc, src, w, h, pitch_y, pitch_c, es)) return e;
    std::vector<uint16_t> packed(entries * 4);
    lut3d_pack(n, table, packed.data());
    if (int e = to_device(dtab, packed.data(), packed.size())) return e;
    const Lut3dArgs a = lut3d_args(f, n, dtab.p, dsrc[0], dsrc[1], dsrc[2], pitch_y, pitch_c, w, h, dst.w, dst.h, out_depth, out_matrix, out_full, dst.p, dst.stride);
    CK(launch_lut3d(0, a, es == 2, sizeof(TO) == 2));
    CK(hipDeviceSynchronize());
    for (int c = 0; c < 3; c++) {
        const auto &pl = dst.planes.p[c];
        CK(hipMemcpy2D(out[c], out_stride[c] * sizeof(TO), pl.pl.p, pl.pl.stride * sizeof(TO), pl.w * sizeof(TO), pl.h, hipMemcpyDeviceToHost));
    }
    return MIHEVC_OK;
}

// the scaling kernel alone
template <typename TO>
int stage_scale(const mihevc_scale_src &f, const void *const *src, int pitch_y, int pitch_c, int dw, int dh, int out_depth, void *const *out)
{
    const size_t es = f.bit_depth > 8 ? 2 : 1;
    ScaleBlock blk;
    if (!scale_block_build(f.width, f.height, dw, dh, SC_TH, SC_ROWS, blk)) return MIHEVC_EINVAL;
    DevBuf din[3], dtab;
    ConvertOut<TO> dst;
    if (int e = dst.alloc(dw, dh)) return e;
    const void *dsrc[3];
    if (int e = upload_yuv420(din, dsrc, src, f.width, f.height, pitch_y, pitch_c, es)) return e;
    if (int e = to_device(dtab, blk.bytes.data(), blk.bytes.size())) return e;
    const int32_t *first[4];
    const int16_t *coef[4];
    tap_pointers(dtab.as<uint8_t>(), blk.first, first); tap_pointers(dtab.as<uint8_t>(), blk.coef, coef);
    const ScaleArgs a = scale_args(f.bit_depth, dsrc[0], dsrc[1], dsrc[2], pitch_y, pitch_c, f.width, f.height, dw, dh, dst.w, dst.h, out_depth, dst.p, dst.stride,
                                   first, coef, blk.taps);
    CK(launch_scale(0, a, es == 2, sizeof(TO) == 2));
    CK(hipDeviceSynchronize());
    return dst.planes.download(out);
}

// the upscaling kernel alone
template <typename TO>
int stage_upscale(const mihevc_upscale_src &f, const void *const *src, int pitch_y, int pitch_c, int dw, int dh, int out_depth, void *const *out)
{
    const size_t es = f.bit_depth > 8 ? 2 : 1;
    UpscaleBlock blk;
    if (!upscale_block_build(f.width, f.height, dw, dh, UP_TH, UP_HALO, UP_ROWS, blk)) return MIHEVC_EINVAL;
    DevBuf din[3], dtab;
    ConvertOut<TO> dst;
    if (int e = dst.alloc(dw, dh)) return e;
    const void *dsrc[3];
    if (int e = upload_yuv420(din, dsrc, src, f.width, f.height, pitch_y, pitch_c, es)) return e;
    if (int e = to_device(dtab, blk.bytes.data(), blk.bytes.size())) return e;
    const int32_t *first[4], *near[4];
    const int16_t *coef[4];
    tap_pointers(dtab.as<uint8_t>(), blk.first, first); tap_pointers(dtab.as<uint8_t>(), blk.near, near); tap_pointers(dtab.as<uint8_t>(), blk.coef, coef);
    const UpscaleArgs a = upscale_args(f, dsrc[0], dsrc[1], dsrc[2], pitch_y, pitch_c, dw, dh, dst.w, dst.h, out_depth, dst.p, dst.stride, first, near, coef);
    CK(launch_upscale(0, a, es == 2, sizeof(TO) == 2));
    CK(hipDeviceSynchronize());
    return dst.planes.download(out);
}

// one convolution alone
int stage_sr_conv(const mihevc_sr_conv_desc &d, const uint16_t *in, const float *weights, const float *bias, const uint16_t *r1, const uint16_t *r2, uint16_t *out)
{
    const int cout_pad = d.planar ? SR_M : d.cout, sw = d.up ? (d.width + 1) / 2 : d.width, sh = d.up ? (d.height + 1) / 2 : d.height;
    const size_t px = (size_t)d.width * d.height, out_n = px * (d.planar ? 3 : d.out_ch);
    std::vector<uint16_t> wpk(sr_packed_halves(cout_pad, d.cin));
    std::vector<float> b((size_t)cout_pad, 0.0f);
    sr_pack_layer(weights, d.cout, d.cin_real, cout_pad, d.cin, wpk.data());
    for (int c = 0; c < d.cout; c++) b[(size_t)c] = bias[c];
    DevBuf din, dw, db, dr1, dr2, dout;
    if (int e = to_device(din, in, (size_t)sw * sh * d.in_ch)) return e;
    if (int e = to_device(dw, wpk.data(), wpk.size())) return e;
    if (int e = to_device(db, b.data(), b.size())) return e;
    if (d.n_res >= 1) if (int e = to_device(dr1, r1, px * d.r1_ch)) return e;
    if (d.n_res >= 2) if (int e = to_device(dr2, r2, px * d.r2_ch)) return e;
    if (int e = to_device(dout, out, out_n)) return e;
    SrConvArgs a;
    a.in = din.as<const uint16_t>(); a.out = dout.as<uint16_t>(); a.wpk = dw.as<const uint16_t>(); a.bias = db.as<const float>();
    a.r1 = dr1.as<const uint16_t>(); a.r2 = dr2.as<const uint16_t>();
    a.in_ch = d.in_ch; a.in_off = d.in_off; a.out_ch = d.out_ch; a.out_off = d.out_off; a.r1_ch = d.r1_ch; a.r1_off = d.r1_off; a.r2_ch = d.r2_ch; a.r2_off = d.r2_off;
    a.w = d.width; a.h = d.height; a.up = d.up; a.act = d.act; a.n_res = d.n_res; a.slope = d.slope; a.a1 = d.a1; a.a2 = d.a2;
    CK(launch_sr_conv(0, a, d.cin, cout_pad, d.planar != 0));
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(out, dout.p, out_n * sizeof(uint16_t), hipMemcpyDeviceToHost));
    return MIHEVC_OK;
}
// the input kernel, and with a network everything behind it
int stage_sr(const mihevc_rgb_format &f, int scale, const SrNet *net, int sw, int sh, const void *const *src, int pitch, uint16_t *out)
{
    const int fct = scale == 2 ? 2 : 1, tw = sw / fct, th = sh / fct;
    DevBuf din[3], arena, dw, db;
    const void *dsrc[3] = {src[0], src[1], src[2]};
    for (int c = 0; c < rgb_planes(f); c++)
        if (int e = upload_as_laid_out(din[c], dsrc[c], rgb_row_elems(f, sw), sh, pitch, (size_t)rgb_elem_size(f))) return e;
    size_t off[SR_BUFS];
    const size_t total = sr_arena_layout(tw, th, off), bytes = net ? total : off[SR_X + 1];
    if (arena.alloc(bytes) != hipSuccess) { (void)hipGetLastError(); return MIHEVC_ENOMEM; }
    CK(launch_sr_input(0, sr_input_args(f, scale, sw, sh, dsrc, pitch, (uint16_t *)(arena.as<uint8_t>() + off[SR_X])), f.sample, rgb_elem_size(f)));
    if (net) {
        if (int e = to_device(dw, net->wpk.data(), net->wpk.size())) return e;
        if (int e = to_device(db, net->bias.data(), net->bias.size())) return e;
        CK(launch_sr_network(0, *net, arena.as<uint8_t>(), dw.as<const uint16_t>(), db.as<const float>(), tw, th));
    }
    CK(hipDeviceSynchronize());
    if (net) CK(hipMemcpy(out, arena.as<uint8_t>() + off[SR_OUT], (size_t)tw * th * 16 * 3 * sizeof(uint16_t), hipMemcpyDeviceToHost));
    else CK(hipMemcpy(out, arena.as<uint8_t>() + off[SR_X], (size_t)tw * th * SR_CIN0 * sizeof(uint16_t), hipMemcpyDeviceToHost));
    return MIHEVC_OK;
}
// one launch of k_sr_compact alone
int stage_sr_compact_conv(const mihevc_sr_compact_conv_desc &d, const uint16_t *in, const float *weights, const float *bias, const float *slopes, const uint16_t *base,
                          uint16_t *out)
{
    const int tail = d.tail ? d.scale : 0, cout = tail ? 3 * tail * tail : 64, cout_pad = (cout + SR_M - 1) / SR_M * SR_M;
    const size_t px = (size_t)d.width * d.height, out_n = px * (tail ? 3 * tail * tail : 64);
    std::vector<uint16_t> wpk(sr_packed_halves(cout_pad, d.cin));
    std::vector<float> par((size_t)cout_pad + 64, 0.0f);
    sr_pack_layer(weights, cout, d.cin_real, cout_pad, d.cin, wpk.data());
    for (int c = 0; c < cout; c++) par[(size_t)c] = bias[c];
    if (!tail) for (int c = 0; c < 64; c++) par[(size_t)cout_pad + c] = slopes[c];
    DevBuf din, dw, dp, dbase, dout;
    if (int e = to_device(din, in, px * d.cin)) return e;
    if (int e = to_device(dw, wpk.data(), wpk.size())) return e;
    if (int e = to_device(dp, par.data(), par.size())) return e;
    if (tail) if (int e = to_device(dbase, base, px * SR_CIN0)) return e;
    if (int e = to_device(dout, out, out_n)) return e;
    SrCompactArgs a;
    a.in = din.as<const uint16_t>(); a.out = dout.as<uint16_t>(); a.wpk = dw.as<const uint16_t>(); a.bias = dp.as<const float>(); a.slope = a.bias + cout_pad;
    a.base = dbase.as<const uint16_t>(); a.w = d.width; a.h = d.height;
    CK(launch_sr_compact(0, a, d.cin, tail));
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(out, dout.p, out_n * sizeof(uint16_t), hipMemcpyDeviceToHost));
    return MIHEVC_OK;
}
// k_sr_input and every launch of a compact network behind it
int stage_sr_compact(const mihevc_rgb_format &f, const SrCompactNet &net, int sw, int sh, const void *const *src, int pitch, uint16_t *out)
{
    DevBuf din[3], arena, dw, dp;
    const void *dsrc[3] = {src[0], src[1], src[2]};
    for (int c = 0; c < rgb_planes(f); c++)
        if (int e = upload_as_laid_out(din[c], dsrc[c], rgb_row_elems(f, sw), sh, pitch, (size_t)rgb_elem_size(f))) return e;
    size_t off[SRC_BUFS];
    const size_t bytes = sr_compact_arena_layout(net.scale, sw, sh, off);
    if (arena.alloc(bytes) != hipSuccess) { (void)hipGetLastError(); return MIHEVC_ENOMEM; }
    CK(launch_sr_input(0, sr_input_args(f, 4, sw, sh, dsrc, pitch, (uint16_t *)(arena.as<uint8_t>() + off[SRC_X])), f.sample, rgb_elem_size(f)));
    if (int e = to_device(dw, net.wpk.data(), net.wpk.size())) return e;
    if (int e = to_device(dp, net.par.data(), net.par.size())) return e;
    CK(launch_sr_compact_network(0, net, arena.as<uint8_t>(), dw.as<const uint16_t>(), dp.as<const float>(), sw, sh));
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(out, arena.as<uint8_t>() + off[SRC_OUT], (size_t)sw * sh * net.scale * net.scale * 3 * sizeof(uint16_t), hipMemcpyDeviceToHost));
    return MIHEVC_OK;
}
// the Y'CbCr input kernel alone
int stage_sr_from_yuv(const mihevc_sr_yuv &f, int scale, const void *const *src, int pitch_y, int pitch_c, uint16_t *out)
{
    const size_t es = f.bit_depth > 8 ? 2 : 1, halves = (size_t)f.width * f.height * SR_CIN0 / (scale == 2 ? 4 : 1);
    DevBuf din[3], dout;
    const void *dsrc[3];
    if (int e = upload_yuv420(din, dsrc, src, f.width, f.height, pitch_y, pitch_c, es)) return e;
    CK(dout.alloc(halves * sizeof(uint16_t)));
    CK(launch_sr_from_yuv(0, sr_yuv_args(f, scale, dsrc[0], dsrc[1], dsrc[2], pitch_y, pitch_c, dout.as<uint16_t>()), es == 2));
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(out, dout.p, halves * sizeof(uint16_t), hipMemcpyDeviceToHost));
    return MIHEVC_OK;
}

// the deinterlacing kernel alone
template <typename T>
int stage_deint(const void *const *prev, const void *const *cur, const void *const *next, int w, int h, int pitch_y, int pitch_c, int depth, int keep, int second,
                void *const *out)
{
    DevBuf din[9];
    ConvertOut<T> dst;
    if (int e = dst.alloc(w, h)) return e;
    const void *d[3][3];
    const void *const *in[3] = {prev, cur, next};
    for (int f = 0; f < 3; f++)
        if (int e = upload_yuv420(din + 3 * f, d[f], in[f], w, h, pitch_y, pitch_c, sizeof(T))) return e;
    const DeintArgs a = deint_args(depth, d[0], d[1], d[2], pitch_y, pitch_c, w, h, dst.w, dst.h, keep, second, dst.p, dst.stride);
    CK(launch_deint(0, a, sizeof(T) == 2));
    CK(hipDeviceSynchronize());
    return dst.planes.download(out);
}

// the denoising kernel alone
template <typename T>
int stage_denoise(const mihevc_denoise &dn, const void *const *prev, const void *const *cur, const void *const *next, int w, int h, int pitch_y, int pitch_c, int depth,
                  void *const *out)
{
    DevBuf din[9];
    ConvertOut<T> dst;
    if (int e = dst.alloc(w, h)) return e;
    const void *d[3][3];
    const void *const *in[3] = {prev, cur, next};
    for (int f = 0; f < 3; f++)
        if (int e = upload_yuv420(din + 3 * f, d[f], in[f], w, h, pitch_y, pitch_c, sizeof(T))) return e;
    const DenoiseArgs a = denoise_args(dn, depth, d[0], d[1], d[2], pitch_y, pitch_c, w, h, dst.w, dst.h, dst.p, dst.stride);
    CK(launch_denoise(0, a, sizeof(T) == 2));
    CK(hipDeviceSynchronize());
    return dst.planes.download(out);
}

// the metrics kernels of inverse telecine alone
template <typename T> int stage_fm_metrics(const void *prev, const void *cur, const void *next, int w, int h, int pitch, int depth, int keep, uint64_t *out)
{
    DevBuf din[3], dpart;
    const void *d[3] = {prev, cur, next};
    for (int f = 0; f < 3; f++)
        if (int e = upload_as_laid_out(din[f], d[f], w, h, pitch, sizeof(T))) return e;
    const size_t n = (size_t)fm_workgroups(w, h);
    CK(dpart.alloc((n + 1) * 8 * sizeof(unsigned long long)));
    unsigned long long *part = dpart.as<unsigned long long>();
    CK(launch_fm_metrics(0, fm_args(depth, d[0], d[1], d[2], pitch, w, h, keep, part), part + n * 8, sizeof(T) == 2));
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(out, part + n * 8, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return MIHEVC_OK;
}
// the weave kernel of inverse telecine alone
template <typename T> int stage_fm_weave(const void *const *cur, const void *const *other, int w, int h, int pitch_y, int pitch_c, int depth, int keep, void *const *out)
{
    DevBuf din[6];
    ConvertOut<T> dst;
    if (int e = dst.alloc(w, h)) return e;
    const void *d[2][3];
    const void *const *in[2] = {cur, other};
    for (int f = 0; f < 2; f++)
        if (int e = upload_yuv420(din + 3 * f, d[f], in[f], w, h, pitch_y, pitch_c, sizeof(T))) return e;
    const DeintArgs a = deint_args(depth, d[1], d[0], d[1], pitch_y, pitch_c, w, h, dst.w, dst.h, keep, 0, dst.p, dst.stride);
    CK(launch_fm_weave(0, a, sizeof(T) == 2));
    CK(hipDeviceSynchronize());
    return dst.planes.download(out);
}

// the vector kernels of frame-rate multiplication alone
template <typename T> int stage_mcfi_vectors(const void *cur, const void *next, int w, int h, int pitch, int depth, int16_t *v0, int16_t *v, uint64_t *scene_sum)
{
    DevBuf din[2], blk;
    const void *d[2] = {cur, next};
    for (int f = 0; f < 2; f++)
        if (int e = upload_as_laid_out(din[f], d[f], w, h, pitch, sizeof(T))) return e;
    const McfiLayout l = mcfi_layout(w, h);
    CK(blk.alloc(l.bytes));
    const McfiSearchArgs a = mcfi_search_args(depth, d[0], d[1], pitch, w, h, blk.as<uint8_t>());
    CK(launch_mcfi_vectors(0, a, mcfi_field_args(a, blk.as<uint8_t>()), sizeof(T) == 2));
    CK(hipDeviceSynchronize());
    const size_t nb = (size_t)mcfi_blocks(w) * mcfi_blocks(h);
    CK(hipMemcpy(v0, blk.as<uint8_t>() + l.v0, nb * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(v, blk.as<uint8_t>() + l.v, nb * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(scene_sum, blk.as<uint8_t>() + l.dsum, 8, hipMemcpyDeviceToHost));
    return MIHEVC_OK;
}
// the render kernel of frame-rate multiplication alone
template <typename T>
int stage_mcfi_render(const mihevc_interpolate &m, int j, const void *const *cur, const void *const *next, const int16_t *v, uint64_t scene_sum, int w, int h, int pitch_y,
                      int pitch_c, int depth, void *const *out)
{
    DevBuf din[6], dv, dsum;
    ConvertOut<T> dst;
    if (int e = dst.alloc(w, h)) return e;
    const void *d[2][3];
    const void *const *in[2] = {cur, next};
    for (int f = 0; f < 2; f++)
        if (int e = upload_yuv420(din + 3 * f, d[f], in[f], w, h, pitch_y, pitch_c, sizeof(T))) return e;
    if (v)
        if (int e = to_device(dv, v, (size_t)mcfi_blocks(w) * mcfi_blocks(h) * 2)) return e;
    const unsigned long long sum = scene_sum;
    if (int e = to_device(dsum, &sum)) return e;
    const McfiRenderArgs a = mcfi_render_args(m, j, depth, d[0], d[1], pitch_y, pitch_c, w, h, dst.w, dst.h, dv.as<int16_t>(), dsum.as<unsigned long long>(), dst.p, dst.stride);
    CK(launch_mcfi_render(0, a, sizeof(T) == 2));
    CK(hipDeviceSynchronize());
    return dst.planes.download(out);
}

// every frame of a stage entry's planar sources is there, with its three planes
bool frames_ok(std::initializer_list<const void *const *> frames)
{
    for (const void *const *f : frames)
        if (!f || !f[0] || !f[1] || !f[2]) return false;
    return true;
}

int select_device(int device)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return MIHEVC_ENODEV;
    if (device < 0 || device >= n) return MIHEVC_EINVAL;
    return hipSetDevice(device) == hipSuccess ? 0 : MIHEVC_EDEVICE;
}

}  // namespace

extern "C" {

int mihevc_device_count(void) { return gfx950_device_count(); }
int mihevc_device_numa_node(int device)
{
    char bus[64] = {0};
    if (device < 0 || device >= gfx950_device_count() || hipDeviceGetPCIBusId(bus, (int)sizeof bus, device) != hipSuccess) return -1;
    for (char *c = bus; *c; c++) if (*c >= 'A' && *c <= 'F') *c = (char)(*c - 'A' + 'a');      // sysfs names are lower case
    char path[160];
    snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", bus);
    FILE *f = fopen(path, "r");
    if (!f) return -1;
    int node = -1;
    if (fscanf(f, "%d", &node) != 1) node = -1;
    fclose(f);
    return node;
}

int mihevc_k_transform_sdh(int device, const int16_t *residual, int16_t *levels, int16_t *recon_residual, int n_blocks, int log2n, int qp,
                           int bit_depth, int intra, int dst4, int scan_idx, int sign_hide)
{
    if (!residual || !levels || !recon_residual || n_blocks <= 0 || log2n < 2 || log2n > 5 || (dst4 && log2n != 2)) return MIHEVC_EINVAL;
    if (scan_idx < 0 || scan_idx > 2 || (sign_hide != 0 && sign_hide != 1)) return MIHEVC_EINVAL;
    if (bit_depth != 8 && bit_depth != 10) return MIHEVC_EINVAL;
    if (int e = select_device(device)) return e;
    const size_t bytes = (size_t)n_blocks << (2 * log2n + 1);
    DevBuf dres, dlvl, drec;
    CK(dres.alloc(bytes)); CK(dlvl.alloc(bytes)); CK(drec.alloc(bytes));
    CK(hipMemcpy(dres.p, residual, bytes, hipMemcpyHostToDevice));
    if (log2n == 2) {     // 4-point DCT, or DST-VII (intra luma 4x4)
        hipLaunchKernelGGL(k_transform4_blocks, dim3((unsigned)((n_blocks + NT / 16 - 1) / (NT / 16))), dim3(NT), 0, 0, dres.as<int16_t>(), dlvl.as<int16_t>(),
                           drec.as<int16_t>(), n_blocks, qp, bit_depth, intra, dst4, scan_idx, sign_hide);
        CK(hipGetLastError());
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(levels, dlvl.p, bytes, hipMemcpyDeviceToHost));
        CK(hipMemcpy(recon_residual, drec.p, bytes, hipMemcpyDeviceToHost));
        return MIHEVC_OK;
    }
    const int per = 1024 >> (2 * log2n);
    hipLaunchKernelGGL(k_transform_blocks, dim3((unsigned)((n_blocks + per - 1) / per)), dim3(NT), 0, 0, dres.as<int16_t>(), dlvl.as<int16_t>(),
                       drec.as<int16_t>(), n_blocks, log2n, qp, bit_depth, intra, scan_idx, sign_hide);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(levels, dlvl.p, bytes, hipMemcpyDeviceToHost));
    CK(hipMemcpy(recon_residual, drec.p, bytes, hipMemcpyDeviceToHost));
    return MIHEVC_OK;
}

int mihevc_k_transform(int device, const int16_t *residual, int16_t *levels, int16_t *recon_residual, int n_blocks, int log2n, int qp,
                       int bit_depth, int intra, int dst4)
{
    return mihevc_k_transform_sdh(device, residual, levels, recon_residual, n_blocks, log2n, qp, bit_depth, intra, dst4, 0, 0);
}

int mihevc_k_intra_frame(int device, const void *sy, const void *su, const void *sv, int w, int h, const mihevc_cost_params *prm, void *ry, void *ru,
                         void *rv, mihevc_cu_rec *cu, int16_t *cy, int16_t *cu_, int16_t *cv, uint64_t *est)
{
    if (!sy || !su || !sv || !prm || !ry || !ru || !rv || !cu || !cy || !cu_ || !cv || !geometry_ok(w, h)) return MIHEVC_EINVAL;
    if (int e = select_device(device)) return e;
    const void *s[3] = {sy, su, sv};
    void *r[3] = {ry, ru, rv};
    int16_t *c[3] = {cy, cu_, cv};
    return with_depth(prm->bit_depth, [&](auto t) { return stage_intra<decltype(t)>(s, w, h, prm, r, cu, c, est); });
}

int mihevc_k_intra_plan(int device, const void *sy, const void *su, const void *sv, int w, int h, const mihevc_cost_params *prm, mihevc_intra_plan *plan)
{
    if (!sy || !su || !sv || !prm || !plan || !geometry_ok(w, h)) return MIHEVC_EINVAL;
    if (prm->tile_cols > ctus_of(w) || prm->tile_rows > ctus_of(h)) return MIHEVC_EINVAL;
    if (prm->bit_depth != 8 && prm->bit_depth != 10) return MIHEVC_EINVAL;
    if (int e = select_device(device)) return e;
    const void *s[3] = {sy, su, sv};
    return with_depth(prm->bit_depth, [&](auto t) { return stage_intra_plan<decltype(t)>(s, w, h, prm, plan); });
}

int mihevc_k_scene_diff(int device, const void *const *luma, const int32_t *pitch, int n, int w, int h, int bit_depth, uint64_t *out)
{
    if (!luma || !pitch || !out || n < 1 || w < 1 || h < 1 || w > 8192 || h > 4352 || (bit_depth != 8 && bit_depth != 10)) return MIHEVC_EINVAL;
    for (int i = 0; i < n; i++)
        if (!luma[i] || pitch[i] < w) return MIHEVC_EINVAL;
    if (int e = select_device(device)) return e;
    return with_depth(bit_depth, [&](auto t) { return stage_scene_diff<decltype(t)>(luma, pitch, n, w, h, out); });
}

int mihevc_k_inter_frame(int device, const void *sy, const void *su, const void *sv, const void *fy, const void *fu, const void *fv, int w, int h,
                         const mihevc_cost_params *prm, const int16_t *centers, void *ry, void *ru, void *rv, mihevc_cu_rec *cu, int16_t *cy,
                         int16_t *cu_, int16_t *cv, int32_t *me_dump, uint64_t *est)
{
    if (!sy || !su || !sv || !fy || !fu || !fv || !prm || !ry || !ru || !rv || !cu || !cy || !cu_ || !cv || !geometry_ok(w, h)) return MIHEVC_EINVAL;
    if (prm->me_range < 1 || prm->me_range > MAX_RANGE) return MIHEVC_EINVAL;
    if (int e = select_device(device)) return e;
    const void *s[3] = {sy, su, sv}, *f[3] = {fy, fu, fv};
    void *r[3] = {ry, ru, rv};
    int16_t *c[3] = {cy, cu_, cv};
    return with_depth(prm->bit_depth, [&](auto t) { return stage_inter<decltype(t)>(s, f, nullptr, w, h, prm, centers, nullptr, r, cu, c, me_dump, nullptr, est); });
}

int mihevc_k_b_frame(int device, const void *sy, const void *su, const void *sv, const void *f0y, const void *f0u, const void *f0v, const void *f1y, const void *f1u,
                     const void *f1v, int w, int h, const mihevc_cost_params *prm, const int16_t *centers0, const int16_t *centers1, void *ry, void *ru, void *rv,
                     mihevc_cu_rec *cu, int16_t *cy, int16_t *cu_, int16_t *cv, int32_t *me_dump0, int32_t *me_dump1, uint64_t *est)
{
    if (!sy || !su || !sv || !f0y || !f0u || !f0v || !f1y || !f1u || !f1v || !prm || !ry || !ru || !rv || !cu || !cy || !cu_ || !cv || !geometry_ok(w, h)) return MIHEVC_EINVAL;
    if (prm->me_range < 1 || prm->me_range > MAX_RANGE) return MIHEVC_EINVAL;
    if (int e = select_device(device)) return e;
    const void *s[3] = {sy, su, sv}, *f0[3] = {f0y, f0u, f0v}, *f1[3] = {f1y, f1u, f1v};
    void *r[3] = {ry, ru, rv};
    int16_t *c[3] = {cy, cu_, cv};
    return with_depth(prm->bit_depth, [&](auto t) { return stage_inter<decltype(t)>(s, f0, f1, w, h, prm, centers0, centers1, r, cu, c, me_dump0, me_dump1, est); });
}

int mihevc_k_deblock(int device, void *ry, void *ru, void *rv, int w, int h, const mihevc_cu_rec *cu, int bit_depth)
{
    if (!ry || !ru || !rv || !cu || !geometry_ok(w, h)) return MIHEVC_EINVAL;
    if (int e = select_device(device)) return e;
    void *r[3] = {ry, ru, rv};
    return with_depth(bit_depth, [&](auto t) { return stage_deblock<decltype(t)>(r, w, h, cu, bit_depth); });
}

int mihevc_k_sao(int device, const void *sy, const void *su, const void *sv, const void *dy, const void *du, const void *dv, int w, int h,
                 const mihevc_cost_params *prm, void *oy, void *ou, void *ov, mihevc_sao_ctu *sao)
{
    if (!sy || !su || !sv || !dy || !du || !dv || !prm || !oy || !ou || !ov || !sao || !geometry_ok(w, h)) return MIHEVC_EINVAL;
    if (int e = select_device(device)) return e;
    const void *s[3] = {sy, su, sv}, *d[3] = {dy, du, dv};
    void *o[3] = {oy, ou, ov};
    return with_depth(prm->bit_depth, [&](auto t) { return stage_sao<decltype(t)>(s, d, w, h, prm, o, sao); });
}

int mihevc_k_loop_filter(int device, const void *sy, const void *su, const void *sv, const void *ry, const void *ru, const void *rv, int w, int h,
                         const mihevc_cu_rec *cu, const mihevc_cost_params *prm, void *oy, void *ou, void *ov, mihevc_sao_ctu *sao)
{
    if (!sy || !su || !sv || !ry || !ru || !rv || !cu || !prm || !oy || !ou || !ov || !sao || !geometry_ok(w, h)) return MIHEVC_EINVAL;
    if (int e = select_device(device)) return e;
    const void *s[3] = {sy, su, sv}, *r[3] = {ry, ru, rv};
    void *o[3] = {oy, ou, ov};
    return with_depth(prm->bit_depth, [&](auto t) { return stage_sao<decltype(t)>(s, r, w, h, prm, o, sao, cu); });
}

int mihevc_k_picture_hash(int device, const void *y, const void *u, const void *v, int w, int h, int bit_depth, int hash_type, void *out)
{
    if (!y || !u || !v || !out || !geometry_ok(w, h) || (bit_depth != 8 && bit_depth != 10) || hash_type < 0 || hash_type > 2) return MIHEVC_EINVAL;
    const void *pl[3] = {y, u, v};
    if (hash_type == 0) {     // MD5: on the host, as a session computes it
        const int bps = bit_depth > 8 ? 2 : 1;
        for (int c = 0; c < 3; c++) {
            const size_t row = (size_t)(c ? w / 2 : w) * bps;
            md5_plane((const uint8_t *)pl[c], row, row, c ? h / 2 : h, (uint8_t *)out + 16 * c);
        }
        return MIHEVC_OK;
    }
    if (int e = select_device(device)) return e;
    return with_depth(bit_depth, [&](auto t) { return stage_picture_hash<decltype(t)>(pl, w, h, hash_type, (uint32_t *)out); });
}

int mihevc_k_ssim(int device, const void *ay, const void *au, const void *av, const void *by, const void *bu, const void *bv, int w, int h, int bit_depth,
                  int64_t sum_q32[3], int64_t windows[3])
{
    if (!ay || !au || !av || !by || !bu || !bv || !sum_q32 || !windows || !geometry_ok(w, h) || (bit_depth != 8 && bit_depth != 10)) return MIHEVC_EINVAL;
    if (int e = select_device(device)) return e;
    const void *a[3] = {ay, au, av}, *b[3] = {by, bu, bv};
    for (int c = 0; c < 3; c++) windows[c] = (int64_t)ssim_windows_x(c ? w / 2 : w) * ssim_windows_y(c ? h / 2 : h);
    if (bit_depth == 8) return stage_ssim<uint8_t>(a, b, w, h, sum_q32);
    return stage_ssim<uint16_t>(a, b, w, h, sum_q32);
}

int mihevc_k_convert_source(int device, const mihevc_src_format *fmt, const void *y, const void *u, const void *v, int width, int height, int pitch_y, int pitch_c,
                            int out_bit_depth, void *out_y, void *out_u, void *out_v)
{
    if (!src_format_ok(fmt) || !y || !u || (!v && !fmt->semi_planar) || !out_y || !out_u || !out_v || !convert_geometry_ok(width, height, out_bit_depth)) return MIHEVC_EINVAL;
    if (pitch_y < width || pitch_c < src_chroma_row(*fmt, width)) return MIHEVC_EINVAL;
    if (int e = select_device(device)) return e;
    const void *src[3] = {y, u, v};
    void *out[3] = {out_y, out_u, out_v};
    return with_depth(out_bit_depth, [&](auto t) { return stage_convert<decltype(t)>(*fmt, src, width, height, pitch_y, pitch_c, out_bit_depth, out); });
}

int mihevc_k_convert_rgb(int device, const mihevc_rgb_format *fmt, const void *p0, const void *p1, const void *p2, int width, int height, int pitch,
                         int out_bit_depth, void *out_y, void *out_u, void *out_v)
{
    if (!rgb_format_ok(fmt) || !rgb_matrix_ok(fmt->matrix) || fmt->range == 0 || !out_y || !out_u || !out_v) return MIHEVC_EINVAL;
    const void *src[3] = {p0, p1, p2};
    if (!rgb_planes_ok(*fmt, src, pitch, width) || !convert_geometry_ok(width, height, out_bit_depth)) return MIHEVC_EINVAL;
    if (int e = select_device(device)) return e;
    void *out[3] = {out_y, out_u, out_v};
    return with_depth(out_bit_depth, [&](auto t) { return stage_convert_rgb<decltype(t)>(*fmt, src, width, height, pitch, out_bit_depth, out); });
}

int mihevc_k_lut3d(int device, const mihevc_lut3d_src *src, int n, const uint16_t *table, const void *y, const void *u, const void *v, int pitch_y, int pitch_c,
                   int width, int height, int out_bit_depth, int out_matrix, int out_full_range, void *const out[3], const int out_stride[3])
{
    if (!lut3d_src_ok(src) || !lut3d_n_ok(n) || !table || !rgb_matrix_ok(out_matrix) || (out_full_range != 0 && out_full_range != 1)) return MIHEVC_EINVAL;
    if (!convert_geometry_ok(width, height, out_bit_depth) || !lut3d_planes_ok(*src, y, u, v, pitch_y, pitch_c, width) || !out || !out_stride) return MIHEVC_EINVAL;
    const int pw = (width + 7) & ~7;
    for (int c = 0; c < 3; c++)
        if (!out[c] || out_stride[c] < (c ? pw / 2 : pw)) return MIHEVC_EINVAL;
    if (int e = select_device(device)) return e;
    const void *p[3] = {y, u, v};
    return with_depth(out_bit_depth, [&](auto t) {
        return stage_lut3d<decltype(t)>(*src, n, table, p, width, height, pitch_y, pitch_c, out_bit_depth, out_matrix, out_full_range != 0, out, out_stride);
    });
}

int mihevc_k_scale_source(int device, const mihevc_scale_src *src, const void *y, const void *u, const void *v, int pitch_y, int pitch_c, int dst_width, int dst_height,
                          int out_bit_depth, void *out_y, void *out_u, void *out_v)
{
    if (!scale_src_ok(src) || !y || !u || !v || !out_y || !out_u || !out_v || !convert_geometry_ok(dst_width, dst_height, out_bit_depth)) return MIHEVC_EINVAL;
    if (!scale_geometry_ok(src->width, src->height, dst_width, dst_height) || src->width > 4 * 8192 || src->height > 4 * 4352) return MIHEVC_EINVAL;
    if (pitch_y < src->width || pitch_c < src->width / 2) return MIHEVC_EINVAL;
    if (int e = select_device(device)) return e;
    const void *p[3] = {y, u, v};
    void *out[3] = {out_y, out_u, out_v};
    return with_depth(out_bit_depth, [&](auto t) { return stage_scale<decltype(t)>(*src, p, pitch_y, pitch_c, dst_width, dst_height, out_bit_depth, out); });
}

int mihevc_k_deinterlace(int device, const void *const prev[3], const void *const cur[3], const void *const next[3], int width, int height, int pitch_y, int pitch_c,
                         int bit_depth, int keep, int second, void *out_y, void *out_u, void *out_v)
{
    if (!frames_ok({prev, cur, next}) || !out_y || !out_u || !out_v) return MIHEVC_EINVAL;
    if (!deint_geometry_ok(width, height) || !convert_geometry_ok(width, height, bit_depth) || pitch_y < width || pitch_c < width / 2) return MIHEVC_EINVAL;
    if ((keep != 0 && keep != 1) || (second != 0 && second != 1)) return MIHEVC_EINVAL;
    if (int e = select_device(device)) return e;
    void *out[3] = {out_y, out_u, out_v};
    return with_depth(bit_depth, [&](auto t) { return stage_deint<decltype(t)>(prev, cur, next, width, height, pitch_y, pitch_c, bit_depth, keep, second, out); });
}

int mihevc_k_denoise(int device, const mihevc_denoise *dn, const void *const prev[3], const void *const cur[3], const void *const next[3], int width, int height,
                     int pitch_y, int pitch_c, int bit_depth, void *out_y, void *out_u, void *out_v)
{
    if (!denoise_strength_ok(dn) || !frames_ok({prev, cur, next}) || !out_y || !out_u || !out_v) return MIHEVC_EINVAL;
    if (!denoise_geometry_ok(width, height) || !convert_geometry_ok(width, height, bit_depth) || pitch_y < width || pitch_c < width / 2) return MIHEVC_EINVAL;
    if (int e = select_device(device)) return e;
    void *out[3] = {out_y, out_u, out_v};
    return with_depth(bit_depth, [&](auto t) { return stage_denoise<decltype(t)>(*dn, prev, cur, next, width, height, pitch_y, pitch_c, bit_depth, out); });
}

int mihevc_k_fieldmatch_metrics(int device, const void *prev_y, const void *cur_y, const void *next_y, int width, int height, int pitch, int bit_depth, int keep,
                                uint64_t out[8])
{
    if (!prev_y || !cur_y || !next_y || !out || !deint_geometry_ok(width, height) || !convert_geometry_ok(width, height, bit_depth) || pitch < width) return MIHEVC_EINVAL;
    if (keep != 0 && keep != 1) return MIHEVC_EINVAL;
    if (int e = select_device(device)) return e;
    return with_depth(bit_depth, [&](auto t) { return stage_fm_metrics<decltype(t)>(prev_y, cur_y, next_y, width, height, pitch, bit_depth, keep, out); });
}

int mihevc_k_fieldmatch_weave(int device, const void *const cur[3], const void *const other[3], int width, int height, int pitch_y, int pitch_c, int bit_depth,
                              int keep, void *out_y, void *out_u, void *out_v)
{
    if (!frames_ok({cur, other}) || !out_y || !out_u || !out_v) return MIHEVC_EINVAL;
    if (!deint_geometry_ok(width, height) || !convert_geometry_ok(width, height, bit_depth) || pitch_y < width || pitch_c < width / 2) return MIHEVC_EINVAL;
    if (keep != 0 && keep != 1) return MIHEVC_EINVAL;
    if (int e = select_device(device)) return e;
    void *out[3] = {out_y, out_u, out_v};
    return with_depth(bit_depth, [&](auto t) { return stage_fm_weave<decltype(t)>(cur, other, width, height, pitch_y, pitch_c, bit_depth, keep, out); });
}

int mihevc_k_mcfi_vectors(int device, const void *cur_y, const void *next_y, int width, int height, int pitch, int bit_depth, int16_t *v0, int16_t *v, uint64_t *scene_sum)
{
    if (!cur_y || !next_y || !v0 || !v || !scene_sum || !mcfi_geometry_ok(width, height) || !convert_geometry_ok(width, height, bit_depth) || pitch < width) return MIHEVC_EINVAL;
    if (int e = select_device(device)) return e;
    return with_depth(bit_depth, [&](auto t) { return stage_mcfi_vectors<decltype(t)>(cur_y, next_y, width, height, pitch, bit_depth, v0, v, scene_sum); });
}

int mihevc_k_mcfi_render(int device, const mihevc_interpolate *d, int j, const void *const cur[3], const void *const next[3], const int16_t *v, uint64_t scene_sum,
                         int width, int height, int pitch_y, int pitch_c, int bit_depth, void *out_y, void *out_u, void *out_v)
{
    if (!mcfi_mode_ok(d) || j < 0 || j >= d->factor || !frames_ok({cur, next}) || !out_y || !out_u || !out_v || (!v && d->mode == 0)) return MIHEVC_EINVAL;
    if (!mcfi_geometry_ok(width, height) || !convert_geometry_ok(width, height, bit_depth) || pitch_y < width || pitch_c < width / 2) return MIHEVC_EINVAL;
    if (v && !mcfi_vectors_ok(v, (size_t)mcfi_blocks(width) * mcfi_blocks(height))) return MIHEVC_EINVAL;
    if (int e = select_device(device)) return e;
    void *out[3] = {out_y, out_u, out_v};
    return with_depth(bit_depth, [&](auto t) { return stage_mcfi_render<decltype(t)>(*d, j, cur, next, v, scene_sum, width, height, pitch_y, pitch_c, bit_depth, out); });
}

int mihevc_k_upscale_source(int device, const mihevc_upscale_src *src, const void *y, const void *u, const void *v, int pitch_y, int pitch_c, int dst_width, int dst_height,
                            int out_bit_depth, void *out_y, void *out_u, void *out_v)
{
    if (!upscale_src_ok(src) || !y || !u || !v || !out_y || !out_u || !out_v || !convert_geometry_ok(dst_width, dst_height, out_bit_depth)) return MIHEVC_EINVAL;
    if (!upscale_geometry_ok(src->width, src->height, dst_width, dst_height)) return MIHEVC_EINVAL;
    if (pitch_y < src->width || pitch_c < src->width / 2) return MIHEVC_EINVAL;
    if (int e = select_device(device)) return e;
    const void *p[3] = {y, u, v};
    void *out[3] = {out_y, out_u, out_v};
    return with_depth(out_bit_depth, [&](auto t) { return stage_upscale<decltype(t)>(*src, p, pitch_y, pitch_c, dst_width, dst_height, out_bit_depth, out); });
}

// what a single k_sr_conv launch can be
static bool sr_conv_desc_ok(const mihevc_sr_conv_desc *d)
{
    if (!d || d->width < 1 || d->height < 1 || d->width > 32768 || d->height > 32768 || (d->up | d->planar | d->act) & ~1 || d->n_res < 0 || d->n_res > 2) return false;
    if (d->planar && d->n_res) return false;      // (the planar instance's 64 lanes would read 16 residual channels; the network's last layer has none)
    if (d->cin < SR_K || d->cin > SR_MAX_CIN || d->cin % SR_K || d->cin_real < 1 || d->cin_real > d->cin) return false;
    if (d->in_ch % 8 || d->in_off % 8 || d->in_off < 0 || d->in_off + d->cin > d->in_ch) return false;
    if (d->planar ? d->cout != 3 || d->cin != 64 : (d->cout != 32 && d->cout != 64) || d->out_ch % 8 || d->out_off % 8 || d->out_off < 0 || d->out_off + d->cout > d->out_ch) return false;
    if (!d->planar && !((d->cout == 64 && (d->cin == 32 || d->cin == 64 || d->cin == 192)) || (d->cout == 32 && d->cin >= 64 && d->cin <= 160))) return false;
    const int c = d->planar ? 8 : d->cout;
    if (d->n_res >= 1 && (d->r1_ch % 8 || d->r1_off % 8 || d->r1_off < 0 || d->r1_off + c > d->r1_ch)) return false;
    if (d->n_res >= 2 && (d->r2_ch % 8 || d->r2_off % 8 || d->r2_off < 0 || d->r2_off + c > d->r2_ch)) return false;
    return true;
}
int mihevc_k_sr_conv(int device, const mihevc_sr_conv_desc *d, const uint16_t *in, const float *weights, const float *bias, const uint16_t *r1, const uint16_t *r2,
                     uint16_t *out)
{
    if (!sr_conv_desc_ok(d) || !in || !weights || !bias || !out || (d->n_res >= 1 && !r1) || (d->n_res >= 2 && !r2)) return MIHEVC_EINVAL;
    if (int e = select_device(device)) return e;
    return stage_sr_conv(*d, in, weights, bias, r1, r2, out);
}

int mihevc_k_sr_input(int device, const mihevc_rgb_format *fmt, int scale, int src_width, int src_height, const void *p0, const void *p1, const void *p2, int pitch,
                      uint16_t *out)
{
    const void *src[3] = {p0, p1, p2};
    if (!rgb_format_ok(fmt) || (scale != 2 && scale != 4) || !sr_geometry_ok(scale, src_width, src_height) || !out || !rgb_planes_ok(*fmt, src, pitch, src_width))
        return MIHEVC_EINVAL;
    if (int e = select_device(device)) return e;
    return stage_sr(*fmt, scale, nullptr, src_width, src_height, src, pitch, out);
}

int mihevc_k_sr_network(int device, const mihevc_sr_model *model, const float *weights, size_t count, const mihevc_rgb_format *fmt, int src_width, int src_height,
                        const void *p0, const void *p1, const void *p2, int pitch, uint16_t *out)
{
    const void *src[3] = {p0, p1, p2};
    if (!sr_model_ok(model) || !weights || count != sr_net_count(model->scale, model->blocks) || !rgb_format_ok(fmt) || !out) return MIHEVC_EINVAL;
    if (!sr_geometry_ok(model->scale, src_width, src_height) || !rgb_planes_ok(*fmt, src, pitch, src_width)) return MIHEVC_EINVAL;
    SrNet net;
    if (!sr_net_build(model->scale, model->blocks, weights, count, net)) return MIHEVC_EINVAL;
    if (int e = select_device(device)) return e;
    return stage_sr(*fmt, model->scale, &net, src_width, src_height, src, pitch, out);
}

int mihevc_k_sr_from_yuv(int device, const mihevc_sr_yuv *src, int scale, const void *y, const void *u, const void *v, int pitch_y, int pitch_c, uint16_t *out)
{
    if (!sr_yuv_src_ok(src) || (scale != 2 && scale != 4) || !out || !sr_yuv_planes_ok(*src, y, u, v, pitch_y, pitch_c)) return MIHEVC_EINVAL;
    if (int e = select_device(device)) return e;
    const void *p[3] = {y, u, v};
    return stage_sr_from_yuv(*src, scale, p, pitch_y, pitch_c, out);
}

// what a single k_sr_compact launch can be
static bool sr_compact_conv_desc_ok(const mihevc_sr_compact_conv_desc *d)
{
    if (!d || d->width < 1 || d->height < 1 || d->width > 8192 || d->height > 8192 || d->tail & ~1 || d->reserved[0] || d->reserved[1]) return false;
    if ((d->cin != 32 && d->cin != 64) || d->cin_real < 1 || d->cin_real > d->cin) return false;
    return !d->tail || (d->cin == 64 && (d->scale == 2 || d->scale == 4));
}
int mihevc_k_sr_compact_conv(int device, const mihevc_sr_compact_conv_desc *d, const uint16_t *in, const float *weights, const float *bias, const float *slopes,
                             const uint16_t *base, uint16_t *out)
{
    if (!sr_compact_conv_desc_ok(d) || !in || !weights || !bias || !out || (d->tail ? !base : !slopes)) return MIHEVC_EINVAL;
    if (int e = select_device(device)) return e;
    return stage_sr_compact_conv(*d, in, weights, bias, slopes, base, out);
}

int mihevc_k_sr_compact_network(int device, const mihevc_sr_compact *model, const float *weights, size_t count, const mihevc_rgb_format *fmt, int src_width,
                                int src_height, const void *p0, const void *p1, const void *p2, int pitch, uint16_t *out)
{
    const void *src[3] = {p0, p1, p2};
    if (!sr_compact_ok(model) || !weights || count != sr_compact_count(model->scale, model->convs) || !rgb_format_ok(fmt) || !out) return MIHEVC_EINVAL;
    if (!sr_compact_geometry_ok(src_width, src_height) || !rgb_planes_ok(*fmt, src, pitch, src_width)) return MIHEVC_EINVAL;
    SrCompactNet net;
    if (!sr_compact_build(model->scale, model->convs, weights, count, net)) return MIHEVC_EINVAL;
    if (int e = select_device(device)) return e;
    return stage_sr_compact(*fmt, net, src_width, src_height, src, pitch, out);
}

#ifdef MIHEVC_PHASE_PROF
// diagnostic build only: read (and optionally clear) the per-call-site cycle table of GpuExec::phase
int mihevc_debug_phase_profile(unsigned long long *out, int reset)
{
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(mihevc::g_phase_prof), sizeof(unsigned long long) * 8 * 1024 * 3) != hipSuccess) return MIHEVC_EDEVICE;
    if (reset) {
        static unsigned long long zero[8 * 1024 * 3];
        if (hipMemcpyToSymbol(HIP_SYMBOL(mihevc::g_phase_prof), zero, sizeof zero) != hipSuccess) return MIHEVC_EDEVICE;
    }
    return MIHEVC_OK;
}
#endif

}  // extern "C"
