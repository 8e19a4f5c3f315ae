// hevc_amd/csrc/device.h — launch layer over the gfx950 kernels (hevc_amd/csrc/kernels/*.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "kernels/common.h"
#include "kernels/deint.h"
#include "kernels/denoise.h"
#include "kernels/fieldmatch.h"
#include "kernels/ingest.h"
#include "kernels/ingest_rgb.h"
#include "kernels/inter.h"
#include "kernels/intra.h"
#include "kernels/loopfilter.h"
#include "kernels/lut3d.h"
#include "kernels/mcfi.h"
#include "kernels/pichash.h"
#include "kernels/scale.h"
#include "kernels/sr_yuv.h"
#include "kernels/ssim.h"
#include "kernels/upscale.h"
#include "sr_net.h"
#include "sr_compact_net.h"

namespace mihevc {

// a device sample plane with an edge border; `pl.p` addresses sample (0,0)
template <typename T> struct DevPlane {
    T *base = nullptr;
    Plane<T> pl{nullptr, 0};
    int w = 0, h = 0, pad = 0;
    size_t bytes() const { return (size_t)pl.stride * (h + 2 * pad) * sizeof(T); }
};
template <typename T> hipError_t alloc_plane(DevPlane<T> &d, int w, int h, int pad);
template <typename T> void free_plane(DevPlane<T> &d);

// Per-picture argument blocks live in device memory (one per picture in flight); launches take an array of them
// and index it with blockIdx.y, so one launch covers every picture of a lock-step batch.
// list 0 / 1: against InterArgs::ref / ref1 (B pictures: the anchor after the picture)
template <typename T> hipError_t launch_me_search(hipStream_t st, const InterArgs<T> *d_args, int n_ctu, int batch, int me_range, int list = 0);
// B pictures: list-0 tree and refinement, list-1 refinement, bi-prediction trial, residual
template <typename T> hipError_t launch_inter_ctu_b(hipStream_t st, const InterArgs<T> *d_args, int n_ctu, int batch, int me_range);
template <typename T> hipError_t launch_inter_ctu(hipStream_t st, const InterArgs<T> *d_args, int n_ctu, int batch, int me_range);
// all anti-diagonals of an I picture batch; h_args is the host copy (geometry only), d_args the device array
// after_plan (optional): recorded between stage A (k_intra_plan, throughput-bound) and the anti-diagonal chain of stage B (latency-bound: other streams' work fits beside it)
template <typename T> hipError_t launch_intra_picture(hipStream_t st, const IntraArgs<T> *d_args, int ctus_w, int ctus_h, int batch, int tile_cols, int tile_rows, hipEvent_t after_plan);
template <typename T> hipError_t launch_intra_p(hipStream_t st, const IntraArgs<T> *d_args, int n_ctu, int batch);
// a whole chunk: d_args[i] = picture i in stream order; its 1/4-size SOURCE picture (lsrc) and its search centres from lsrc against lref (the predecessor's lsrc)
template <typename T> hipError_t launch_pre_search_chunk(hipStream_t st, const PreArgs<T> *d_args, int w, int h, int n_ctu, int n_pictures);
// with_lowres false: the 1/4-size pictures were made by launch_prep_p_step
template <typename T> hipError_t launch_pre_search(hipStream_t st, const PreArgs<T> *d_args, int w, int h, int n_ctu, int batch, bool with_lowres);
template <typename T> hipError_t launch_deblock(hipStream_t st, const DeblockArgs<T> *d_args_v, const DeblockArgs<T> *d_args_h, int w, int h, int batch);
template <typename T> hipError_t launch_sao(hipStream_t st, const SaoArgs<T> *d_args, int w, int h, int batch, bool decide);
template <typename T> hipError_t launch_pad(hipStream_t st, const SaoArgs<T> *d_args, int w, int h, int batch);
// per-picture sum of squared error into args.sse[0..2] (u64, accumulated with atomics: zero the targets first)
template <typename T> hipError_t launch_frame_sse(hipStream_t st, const SaoArgs<T> *d_args, int batch);
template <typename T> hipError_t launch_sse_fold(hipStream_t st, const SaoArgs<T> *d_args, int n_ctu, int batch);
// decoded picture hash (kernels/pichash.h) of the final reconstructions SaoArgs::out, coded size, every picture of the batch: kind 1 CRC, 2 checksum.
// The three 32-bit hash words go to (uint8_t *)args.sse + out_off; `part` is scratch of pic_hash_part_words(w, h, sizeof(T)) words per picture
int pic_hash_part_words(int w, int h, int bps);
template <typename T> hipError_t launch_pic_hash(hipStream_t st, const SaoArgs<T> *d_args, int w, int h, int batch, int kind, uint32_t *part, size_t out_off);
// SSIM (kernels/ssim.h) of the sources SaoArgs::src against the final reconstructions SaoArgs::out, coded size, every picture of the batch: the three int64
// sums of Q go to (uint8_t *)args.sse + out_off (8-byte aligned); `part` is scratch of ssim_part_words(w, h) int64 per picture
int ssim_part_words(int w, int h);
template <typename T> hipError_t launch_ssim(hipStream_t st, const SaoArgs<T> *d_args, int w, int h, int batch, long long *part, size_t out_off);
constexpr int MAX_LANES = 16;
struct StepParams { CostParams prm[MAX_LANES]; int p_tile_cols, p_tile_rows; };      // one P step's cost parameters per lane, passed by value; the P pictures' tile grid (intra second pass: availability)
// head of a P step in one launch: border pad of the pictures `prev` describes (nullptr: none), 1/4-size pictures for `pre` (nullptr: none), then the step's
// cost parameters (by value in `p`) into the lanes' argument blocks, and the four accumulators at SaoArgs::sse zeroed
template <typename T> hipError_t launch_prep_p_step(hipStream_t st, const SaoArgs<T> *prev, const PreArgs<T> *pre, IntraArgs<T> *ia, InterArgs<T> *ea, SaoArgs<T> *sa,
                                                    const StepParams &p, int w, int h, int batch);

// scene-cut detector input: luma plane of one source picture
template <typename T> struct ScenePic { const T *p; int stride; };
template <typename T> hipError_t launch_scene_diff(hipStream_t st, const ScenePic<T> *pics, unsigned long long *out, int w, int h, int n);

template <typename T> hipError_t launch_extend_margin(hipStream_t st, Plane<T> p, int sw, int sh, int pw, int ph);

// source conversion (kernels/ingest.h): one launch writes the three coded-size planes of `a`, margins included.  in16 / out16: uint16 source elements / output samples
hipError_t launch_ingest(hipStream_t st, const IngestArgs &a, bool in16, bool out16);
// RGB source conversion (kernels/ingest_rgb.h).  sample: mihevc_rgb_format::sample; elem_size: bytes of a source element
hipError_t launch_ingest_rgb(hipStream_t st, const IngestRgbArgs &a, int sample, int elem_size, bool out16);
// colour table (kernels/lut3d.h): one launch writes the three coded-size planes of a.out, margins included.  in16 / out16: uint16 source elements / output samples
hipError_t launch_lut3d(hipStream_t st, const Lut3dArgs &a, bool in16, bool out16);
// downscaling source (kernels/scale.h): one launch writes the three coded-size planes of `a`, margins included, from a source of another size
hipError_t launch_scale(hipStream_t st, const ScaleArgs &a, bool in16, bool out16);
// upscaling source (kernels/upscale.h): one launch writes the three coded-size planes of `a`, margins included, from a smaller source
hipError_t launch_upscale(hipStream_t st, const UpscaleArgs &a, bool in16, bool out16);
// learned super-resolution (kernels/sr_conv.h).  One convolution: cin, cout as padded (cin a multiple of 32 up to 192; cout 32 or 64, planar: 16); a shape
// the network has no instance for is hipErrorInvalidValue, never another path
hipError_t launch_sr_conv(hipStream_t st, const SrConvArgs &a, int cin, int cout, bool planar);
// the source -> the input tensor.  sample: mihevc_rgb_format::sample; elem_size: bytes of a source element
hipError_t launch_sr_input(hipStream_t st, const SrInputArgs &a, int sample, int elem_size);
// every launch of `net` (sr_net.h) over an arena and packed weights in device memory; the input tensor of tw x th pixels is in the arena's X
hipError_t launch_sr_network(hipStream_t st, const SrNet &net, uint8_t *arena, const uint16_t *wpk, const float *bias, int tw, int th);
// compact networks (kernels/sr_compact.h).  One layer: cin 32 or 64 as padded; tail 0 (64 channels, PReLU) or the scale of the shuffling last layer (cin 64); a
// shape without an instance is hipErrorInvalidValue, never another kernel
hipError_t launch_sr_compact(hipStream_t st, const SrCompactArgs &a, int cin, int tail);
// every launch of `net` (sr_compact_net.h) over an arena and packed weights in device memory; the input tensor of sw x sh pixels is in the arena's X
hipError_t launch_sr_compact_network(hipStream_t st, const SrCompactNet &net, uint8_t *arena, const uint16_t *wpk, const float *par, int sw, int sh);
// a planar 4:2:0 Y'CbCr source -> the input tensor (kernels/sr_yuv.h).  in16: the source's elements are uint16
hipError_t launch_sr_from_yuv(hipStream_t st, const SrYuvArgs &a, bool in16);
// deinterlacing source (kernels/deint.h): one launch writes the three coded-size planes of `a`, margins included, from three frames at the output's own depth
hipError_t launch_deint(hipStream_t st, const DeintArgs &a, bool is16);
// denoising source (kernels/denoise.h): one launch writes the three coded-size planes of `a`, margins included, from three frames at the output's own depth
hipError_t launch_denoise(hipStream_t st, const DenoiseArgs &a, bool is16);
// inverse telecine (kernels/fieldmatch.h).  Metrics: k_fm_metrics over the luma tiles of `a` into a.part, then k_fm_fold into out[8] (device memory; nothing
// to zero in front).  Weave: one launch writes the three coded-size planes of `a` (cur: the kept rows, prev: the others), margins included
hipError_t launch_fm_metrics(hipStream_t st, const FmArgs &a, unsigned long long *out, bool is16);
hipError_t launch_fm_weave(hipStream_t st, const DeintArgs &a, bool is16);
// frame-rate multiplication (kernels/mcfi.h).  Vectors: k_mcfi_search over the block tiles of `a`, then k_mcfi_field (median, fallback, the fold of D) into
// f.v and f.dsum (device memory; nothing to zero in front).  Render: one launch writes the three coded-size planes of `a`, margins included
hipError_t launch_mcfi_search(hipStream_t st, const McfiSearchArgs &a, bool is16);
hipError_t launch_mcfi_field(hipStream_t st, const McfiFieldArgs &f, bool is16);
hipError_t launch_mcfi_vectors(hipStream_t st, const McfiSearchArgs &a, const McfiFieldArgs &f, bool is16);      // the two above, in this order
hipError_t launch_mcfi_render(hipStream_t st, const McfiRenderArgs &a, bool is16);

// rows between the slices of one picture (csrc/slice_group.h): jobs[i] for i < n_jobs, one grid row of `blocks_per_job` workgroups each
hipError_t launch_copy_rows(hipStream_t st, const RowCopy *d_jobs, int n_jobs, int blocks_per_job);

int gfx950_device_count();

}  // namespace mihevc
