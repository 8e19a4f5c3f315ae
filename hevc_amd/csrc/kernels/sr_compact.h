// hevc_amd/csrc/kernels/sr_compact.h — learned super-resolution with a compact network (SRVGGNetCompact: realesr-animevideov3, realesr-general-x4v3 and its
// denoise partner; mihevc_set_sr_compact, mihevc_k_sr_compact_conv, mihevc_k_sr_compact_network): the one kernel such a network needs behind k_sr_input /
// k_sr_from_yuv.  The numerical definition is DESIGN.md §6m (normative); csrc/sr_compact_net.h packs the weights and lists the launches.
//   tensors     IEEE halves, NHWC, 16-byte aligned: the input tensor X has SR_CIN0 = 32 channels (3 real), every other tensor 64
//   layer       out[y][x][co] = P(bias[co] + sum over ky, kx, ci of in[y + ky - 1][x + kx - 1][ci] W[co][ci][ky][kx]), zero outside the picture; P in fp32:
//               v >= 0 ? v : slope[co] v (one slope per channel), rounded to half (nearest even) once.  Products of halves are summed in fp32 by the MFMA
//   tail        the last layer, 64 -> 3 r r channels (r = 4 or 2), no activation: v = acc + bias[co] + X[y][x][c] with co = c r r + dy r + dx, rounded to half
//               once and stored in plane c of three planes of r h x r w halves at (r y + dy, r x + dx): the pixel-shuffle and the sum with the source
//               enlarged by nearest, in the store
// k_sr_compact is an implicit GEMM on v_mfma_f32_16x16x32_f16 with the operand roles of k_sr_conv (sr_conv.h): the weights are the A operand, 16 adjacent
// pixels of a row the B operand, so a lane's four results are four adjacent channels of one pixel.  In a plain layer that is one 8-byte store; in the tail at
// r = 4 the four are dx = 0 .. 3 of one output row (lane >> 4 is dy, the fragment is the plane): one 8-byte store; at r = 2 the 12 channels are one fragment
// padded to 16, lane >> 4 is the plane and the four are a 2 x 2 block: two 4-byte stores.  What it does that k_sr_conv does not ("what would
// have to change"):
//   weights     every layer here has at most 64 input channels, so a layer's packed weights (73,728 bytes at 64 -> 64) fit in LDS beside a pixel tile.  A
//               workgroup copies them from global memory ONCE, linearly, and then walks tiles wg, wg + n, wg + 2 n .. of the picture with them (n workgroups,
//               at most SRC_MAX_WG = one per CU): no wave fetches a weight from global memory in the loop, and a weight fragment is one conflict-free
//               ds_read_b128 (64 lanes, 64 adjacent 16-byte slots)
//   pixel tile  two images in LDS, taken in turn: while the waves of a workgroup finish a tile (epilogue and stores), each lane already has the next tile's
//               loads in flight and writes them into the other image before the phase's barrier, so a tile costs one wait for memory, not a wait for the fill
//               and another for the stores.  An image is chunk-major: the 16 bytes of channels 8 c .. 8 c + 7 of halo pixel p lie at in[c][p], SRC_NP = 336 slots per chunk (a multiple of 16).  The
//               lanes that ds_read_b128 serves together hold 8 pixels of chunk c and the other 8 of chunk c ^ 1 of one row; their slots are p0 + i, i = 0 .. 15,
//               modulo 16 because SRC_NP is 0 modulo 16: sixteen different 16-byte slots of the 256-byte bank row, for every tap and row.  The fill writes
//               8 adjacent pixels of one chunk per ds_write_b128 group and still loads whole 128-byte pixels per wave instruction
//   steps       step s = tap * CIN / 32 + chunk; CIN / 32 is 1 or 2, so tap = s >> 0 or 1, ky = (0x2A540 >> 2 tap) & 3 (a table of nine 2-bit entries in a
//               constant), kx = tap - 3 ky: no division in the walk
// Budget (NT = 256 lanes: four waves, one per SIMD).  The tile is SRC_TW x SRC_TH = 16 x 16 pixels, a wave takes SRC_ROWS = 4 rows: per step 4 weight and 4
// pixel fragments (8 ds_read_b128) feed 16 MFMAs, twice the MFMAs per LDS read of a 2-row wave, and 64 accumulator registers.  LDS at 64 -> 64:
// 73,728 (weights) + 2 x 8 x 336 x 16 = 86,016 (two tile images with their halo) + 512 (biases and slopes) = 160,256 of the CU's 163,840 bytes, so ONE
// workgroup per CU (SRC_PER_CU; the launch bound allows 512 registers, the kernels take far fewer: tests/test_sr_compact_resources.py prints them).
// 32 -> 64: 36,864 + 43,008 + 512; tail r = 4: 55,296 + 86,016 + 512; r = 2: 18,432 + 86,016 + 512.  No scratch.  One workgroup per CU and one wave per SIMD mean that nothing hides a memory latency but the
// wave's own instructions: the fill issues all of a lane's loads (at most 11, the weights' 18) before it waits for the first, and the epilogue finds biases and
// slopes in LDS; the next tile's fill overlaps this tile's epilogue, but nothing overlaps it with the products (DESIGN.md §6m has the measurements).
// The stepped run (tests/emu/sr_compact.cpp) proves the tiling, the addressing and the stores; only the device run proves the lane maps.
// Out of scope: scale 3 and 1, num_feat other than 64, fusing layers into one launch, fp8 / int8, tiling a frame, batching frames.
#pragma once
#include "sr_conv.h"

namespace mihevc {

constexpr int SRC_TW = 16, SRC_TH = 16;                     // the tile: 16 pixels are the columns of one MFMA
constexpr int SRC_HW = SRC_TW + 2, SRC_HH = SRC_TH + 2;     // with the halo
constexpr int SRC_ROWS = SRC_TH / (NT / 64);                // rows per wave: 4
constexpr int SRC_NP = (SRC_HW * SRC_HH + 15) & ~15;        // 16-byte slots per chunk of the tile image: 336
constexpr int SRC_MAX_WG = 256;                             // workgroups of a launch: one per CU
constexpr int SRC_PER_CU = 1;                               // the second launch bound
typedef uint32_t sr_u32 __attribute__((may_alias));         // two halves stored at once

template <int CIN, int NA> struct SrCompactShared {
    uint8_t w[9 * (CIN / SR_K) * NA * 64][16];              // the packed layer, sr_pack_layer's order: [step][fragment][lane]
    uint8_t in[2][CIN / 8][SRC_NP][16];                     // two images, taken in turn: [chunk of 8 channels][halo pixel]
    float par[128];                                         // the biases (16 NA), from 64 on the slopes
};

struct SrCompactArgs {
    const uint16_t *in;             // CIN channels
    uint16_t *out;                  // 64 channels NHWC, or (tail) the first of three planes of r h x r w
    const uint16_t *wpk;            // packed weights of the layer
    const float *bias;              // 16 NA of them
    const float *slope;             // 64 (not read by the tail)
    const uint16_t *base;           // tail: the input tensor X, SR_CIN0 channels
    int w, h;                       // of the layer's input and output tensors
};

HDI int sr_compact_tiles(int w, int h) { return ((w + SRC_TW - 1) / SRC_TW) * ((h + SRC_TH - 1) / SRC_TH); }
HDI int sr_compact_workgroups(int w, int h) { const int t = sr_compact_tiles(w, h); return t < SRC_MAX_WG ? t : SRC_MAX_WG; }

// workgroup `wg` of `nwg`.  NA: fragments of 16 output channels; TAIL: 0 (64 channels, PReLU), 4 (NA 3) or 2 (NA 1): the scale of the shuffling last layer
template <int CIN, int NA, int TAIL, class Ex> DEV void sr_compact_program(Ex &ex, SrCompactShared<CIN, NA> &s, const SrCompactArgs &a, int wg, int nwg)
{
    static_assert((CIN == 32 || CIN == 64) && (TAIL == 0 ? NA == 4 : TAIL == 4 ? NA == 3 && CIN == 64 : TAIL == 2 && NA == 1 && CIN == 64), "shape");
    constexpr int KC = CIN / SR_K, KSH = KC == 2 ? 1 : 0, CHUNKS = CIN / 8, PPB = 64 / CHUNKS;      // PPB: pixels a wave fills per instruction
    constexpr int WSLOTS = 9 * KC * NA * 64, HALO = SRC_HW * SRC_HH, FILL = (HALO + PPB - 1) / PPB * 64;
    constexpr int WITER = (WSLOTS + NT - 1) / NT, FITER = (FILL + NT - 1) / NT;      // loads a lane has in flight: at most 18 and 11
    const int w = a.w, h = a.h;
    const int ntx = (w + SRC_TW - 1) / SRC_TW, tiles = ntx * ((h + SRC_TH - 1) / SRC_TH);
    if (wg >= tiles) return;
    const uint16_t *const wpk = a.wpk;
    const float *const bias = a.bias, *const slope = a.slope;
    ex.phase([&](int tid) {          // the layer's weights, biases and slopes, once: every load is issued before the first store waits for one
        mfma_frag v[WITER];
#pragma unroll
        for (int k = 0; k < WITER; k++) {
            const int i = tid + k * NT;
            v[k] = *(const mfma_frag *)__builtin_assume_aligned(wpk + (ptrdiff_t)(i < WSLOTS ? i : WSLOTS - 1) * 8, 16);
        }
        if (tid < NA * SR_M) s.par[tid] = bias[tid];
        if (TAIL == 0 && tid < 64) s.par[64 + tid] = slope[tid];
#pragma unroll
        for (int k = 0; k < WITER; k++) {
            const int i = tid + k * NT;
            if (i < WSLOTS) *(mfma_frag *)__builtin_assume_aligned(&s.w[i][0], 16) = v[k];
        }
    });
    const uint16_t *const in = a.in;
    uint16_t *const out = a.out;
    const uint16_t *const base = a.base;
    // The tile `tile` with its halo into image `buf`, in two halves.  64 lanes take PPB adjacent halo pixels, lane j pixel j % PPB and chunk j / PPB.  fill_load
    // issues all of a lane's loads, from addresses clamped into the picture so that none hangs on a branch, and puts the padding's zeros in; fill_store writes
    // them to LDS, which is where the lane first waits
    auto fill_load = [&](int tid, int tile, mfma_frag (&v)[FITER]) {
        const int ty = tile / ntx, tx = tile - ty * ntx, x_base = tx * SRC_TW, y_base = ty * SRC_TH;
#pragma unroll
        for (int k = 0; k < FITER; k++) {
            const int i = tid + k * NT, j = i & 63, q = (i >> 6) * PPB + (j & (PPB - 1)), p = q < HALO ? q : HALO - 1, c = j / PPB;
            const int py = p / SRC_HW, y = y_base - 1 + py, x = x_base - 1 + (p - py * SRC_HW);
            const int yc = y < 0 ? 0 : y < h ? y : h - 1, xc = x < 0 ? 0 : x < w ? x : w - 1;
            v[k] = *(const mfma_frag *)__builtin_assume_aligned(in + ((ptrdiff_t)yc * w + xc) * CIN + c * 8, 16);
            if (yc != y || xc != x) v[k] = mfma_frag{0u, 0u, 0u, 0u};
        }
    };
    auto fill_store = [&](int tid, int buf, const mfma_frag (&v)[FITER]) {
#pragma unroll
        for (int k = 0; k < FITER; k++) {
            const int i = tid + k * NT, j = i & 63, p = (i >> 6) * PPB + (j & (PPB - 1)), c = j / PPB;
            if (p < HALO) *(mfma_frag *)__builtin_assume_aligned(&s.in[buf][c][p][0], 16) = v[k];
        }
    };
    ex.phase([&](int tid) {
        mfma_frag v[FITER];
        fill_load(tid, wg, v);
        fill_store(tid, 0, v);
    });
    int buf = 0;
    for (int tile = wg; tile < tiles; tile += nwg, buf ^= 1) {
        const int ty = tile / ntx, tx = tile - ty * ntx, x_base = tx * SRC_TW, y_base = ty * SRC_TH, next = tile + nwg;
        ex.template mfma_phase<NA, SRC_ROWS>(9 * KC,
            [&](int tid, int step, mfma_frag (&fw)[NA], mfma_frag (&fp)[SRC_ROWS]) {
                const int lane = tid & 63, row0 = (tid >> 6) * SRC_ROWS, tap = step >> KSH, kc = step & (KC - 1), ky = (0x2A540 >> (2 * tap)) & 3, kx = tap - 3 * ky;
#pragma unroll
                for (int m = 0; m < SRC_ROWS; m++)
                    fp[m] = *(const mfma_frag *)__builtin_assume_aligned(&s.in[buf][kc * 4 + (lane >> 4)][(row0 + m + ky) * SRC_HW + (lane & 15) + kx][0], 16);
#pragma unroll
                for (int n = 0; n < NA; n++) fw[n] = *(const mfma_frag *)__builtin_assume_aligned(&s.w[(step * NA + n) * 64 + lane][0], 16);
            },
            [&](int tid, const mfma_acc (&acc)[NA][SRC_ROWS]) {
                // the next tile's loads travel while this tile's results are worked out and stored; its image is the one nobody reads in this phase
                mfma_frag nv[FITER];
                if (next < tiles) fill_load(tid, next, nv);
                const int lane = tid & 63, x = x_base + (lane & 15), g = lane >> 4;
#pragma unroll
                for (int m = 0; m < SRC_ROWS; m++) {
                    const int y = y_base + (tid >> 6) * SRC_ROWS + m;
                    if (y >= h || x >= w) continue;
                    const ptrdiff_t pix = (ptrdiff_t)y * w + x;
                    if constexpr (TAIL == 0) {
#pragma unroll
                        for (int n = 0; n < NA; n++) {
                            const int co = n * SR_M + 4 * g;
                            uint32_t hv[4];
#pragma unroll
                            for (int i = 0; i < 4; i++) {
                                float v = acc[n][m][i] + s.par[co + i];
                                v = v >= 0.0f ? v : s.par[64 + co + i] * v;
                                hv[i] = sr_half_of_float(v);
                            }
                            const ingest_u32x2 o = {hv[0] | hv[1] << 16, hv[2] | hv[3] << 16};
                            *(ingest_u32x2 *)__builtin_assume_aligned(out + pix * 64 + co, 8) = o;
                        }
                    } else if constexpr (TAIL == 4) {      // fragment n is plane n, g is dy, the four results are dx = 0 .. 3
                        const ptrdiff_t ow = (ptrdiff_t)4 * w, plane = ow * 4 * h, at = ((ptrdiff_t)4 * y + g) * ow + 4 * x;
#pragma unroll
                        for (int n = 0; n < NA; n++) {
                            const float b = half_bits_to_float(base[pix * SR_CIN0 + n]);
                            uint32_t hv[4];
#pragma unroll
                            for (int i = 0; i < 4; i++) hv[i] = sr_half_of_float(acc[n][m][i] + s.par[n * SR_M + 4 * g + i] + b);
                            const ingest_u32x2 o = {hv[0] | hv[1] << 16, hv[2] | hv[3] << 16};
                            *(ingest_u32x2 *)__builtin_assume_aligned(out + n * plane + at, 8) = o;
                        }
                    } else {                               // one fragment: g is the plane (3: padding), the four results are (dy, dx) = (0, 0), (0, 1), (1, 0), (1, 1)
                        if (g == 3) continue;
                        const ptrdiff_t ow = (ptrdiff_t)2 * w, plane = ow * 2 * h, at = (ptrdiff_t)2 * y * ow + 2 * x;
                        const float b = half_bits_to_float(base[pix * SR_CIN0 + g]);
                        uint32_t hv[4];
#pragma unroll
                        for (int i = 0; i < 4; i++) hv[i] = sr_half_of_float(acc[0][m][i] + s.par[4 * g + i] + b);
                        *(sr_u32 *)__builtin_assume_aligned(out + g * plane + at, 4) = hv[0] | hv[1] << 16;
                        *(sr_u32 *)__builtin_assume_aligned(out + g * plane + at + ow, 4) = hv[2] | hv[3] << 16;
                    }
                }
                if (next < tiles) fill_store(tid, buf ^ 1, nv);
            });
    }
}

}  // namespace mihevc
