// hevc_amd/csrc/kernels/ctu_image.h — the LDS picture of one CTU that every CTU program works on (intra plan, intra code, NxN, inter, loop filter).
//
// A CTU image is an array of CTU_SAMPLES = 1536 samples (or residuals, levels, descriptors: one entry per sample): plane 0, luma, 32 x 32 at 0 with row
// stride 32; plane 1, Cb, 16 x 16 at 1024 and plane 2, Cr, 16 x 16 at 1280, both with row stride 16.  Its CTU_SUBBLOCKS = 96 4x4 sub-blocks are numbered
// luma first (64, raster order over the 8 x 8 grid), then Cb (16, raster over 4 x 4), then Cr.  The 4 x 4 grid of 8x8 luma tiles (4x4 chroma tiles) is what
// tu_log2 / cbf / cu_acc are indexed by: tile = (y >> 3) * 4 + (x >> 3) in luma, (y >> 2) * 4 + (x >> 2) in chroma coordinates.
// This header is the one definition of that format; nothing else spells the arithmetic out.
#pragma once
#include "common.h"

namespace mihevc {

constexpr int CTU_LUMA = CTU * CTU, CTU_CHROMA = CTU_LUMA / 4;      // samples of the luma plane / of one chroma plane
constexpr int CTU_SAMPLES = CTU_LUMA + 2 * CTU_CHROMA;              // 1536
constexpr int CTU_SUBBLOCKS = CTU_SAMPLES / 16;                     // 96
constexpr int CU8_SAMPLES = 64 + 16 + 16;                           // one 8x8 CU: Y 8x8, Cb 4x4, Cr 4x4

// one sample of the image: coordinates inside its plane (luma 0..31, chroma 0..15), the plane's row stride and base offset
struct CtuSample { int plane, x, y, stride, base; };
DEV int ctu_index(int plane, int x, int y) { return plane ? CTU_LUMA + (plane - 1) * CTU_CHROMA + y * 16 + x : y * 32 + x; }
DEV CtuSample ctu_sample(int idx)
{
    CtuSample c;
    if (idx < CTU_LUMA) { c.plane = 0; c.x = idx & 31; c.y = idx >> 5; c.stride = 32; c.base = 0; }
    else { int i = idx - CTU_LUMA; c.plane = 1 + (i >> 8); i &= 255; c.x = i & 15; c.y = i >> 4; c.stride = 16; c.base = CTU_LUMA + (c.plane - 1) * CTU_CHROMA; }
    return c;
}
// a luma coordinate or size (CTU origin, picture width ...) in the units of `plane`: 4:2:0 chroma is half of it
DEV int to_plane(int plane, int v) { return plane ? v >> 1 : v; }

// 4x4 sub-block sb: its plane, origin (bx, by) in the plane, the plane's stride, the offset `at` of its first sample in the image and the tile that owns it
struct SubBlock { int plane, bx, by, stride, at, tile; };
DEV SubBlock sub_block(int sb)
{
    SubBlock b;
    b.plane = sb < 64 ? 0 : 1 + ((sb - 64) >> 4);
    const int k = sb < 64 ? sb : (sb - 64) & 15, per = b.plane ? 4 : 8, sh = b.plane ? 2 : 3;
    b.bx = (k & (per - 1)) * 4; b.by = (k >> sh) * 4; b.stride = b.plane ? 16 : 32;
    b.at = (b.plane ? CTU_LUMA + (b.plane - 1) * CTU_CHROMA : 0) + b.by * b.stride + b.bx;
    b.tile = (b.by >> sh) * 4 + (b.bx >> sh);
    return b;
}

// lane 0 .. CU8_SAMPLES - 1 of the 8x8 CU at luma (cx, cy): 64 luma samples in raster order, then its 4x4 Cb and 4x4 Cr blocks
DEV CtuSample cu8_sample(int cx, int cy, int lane)
{
    if (lane < 64) return ctu_sample(ctu_index(0, cx + (lane & 7), cy + (lane >> 3)));
    const int k = lane - 64;
    return ctu_sample(ctu_index(1 + (k >> 4), (cx >> 1) + (k & 3), (cy >> 1) + ((k >> 2) & 3)));
}

// the CU_CBF_* flags of the CU whose first tile is t0, from the per-plane tile words (bit t: tile t's TU has a non-zero level)
DEV int cbf_flags(const unsigned (&cbf)[3], int t0)
{
    return ((cbf[0] >> t0) & 1 ? CU_CBF_Y : 0) | ((cbf[1] >> t0) & 1 ? CU_CBF_CB : 0) | ((cbf[2] >> t0) & 1 ? CU_CBF_CR : 0);
}

// the workgroup's CTU source image (zero outside the picture) — dword loads for whole CTUs, all of a lane's
// loads in flight together; sample-wise only for the partial CTUs at the right / bottom picture edge
template <typename T>
DEV void load_ctu_source(T *dst, const Plane<const T> (&src)[3], int x0, int y0, int w, int h, int tid)
{
    constexpr int per = 4 / (int)sizeof(T);
    if (x0 + CTU <= w && y0 + CTU <= h) {
        constexpr int ND = CTU_SAMPLES / per, IT = (ND + NT - 1) / NT;
        uint32_t v[IT];
#pragma unroll
        for (int k = 0; k < IT; k++) {
            const int d = tid + k * NT;
            if (d < ND) {
                const CtuSample c = ctu_sample(d * per);
                v[k] = load_u32(src[c.plane].p + (size_t)(to_plane(c.plane, y0) + c.y) * src[c.plane].stride + to_plane(c.plane, x0) + c.x);
            }
        }
#pragma unroll
        for (int k = 0; k < IT; k++) {
            const int d = tid + k * NT;
            if (d < ND) __builtin_memcpy(__builtin_assume_aligned(dst + d * per, 4), &v[k], 4);
        }
        return;
    }
    for (int i = tid; i < CTU_SAMPLES; i += NT) {
        const CtuSample c = ctu_sample(i);
        const int gx = to_plane(c.plane, x0) + c.x, gy = to_plane(c.plane, y0) + c.y;
        dst[i] = (gx < to_plane(c.plane, w) && gy < to_plane(c.plane, h)) ? src[c.plane].p[(size_t)gy * src[c.plane].stride + gx] : (T)0;
    }
}

}  // namespace mihevc
