// hevc_amd/csrc/kernels/mcfi.h — frame-rate multiplication by motion-compensated interpolation (mihevc_send_frame_interpolate, mihevc_k_mcfi_vectors,
// mihevc_k_mcfi_render): two progressive frames C (frame k) and N (frame k + 1), planar 4:2:0 at the session's own depth B (8 or 10) -> picture j of f
// (f in {2, 3, 4}, j = 0 .. f - 1) between them, in the session's planes, margin included.  Integers only, so that the device, the stepped kernels
// (tests/emu/mcfi.cpp) and the numpy model (tests/mcfi_ref.py) agree bit for bit.  The definition (normative: DESIGN.md §6j):
//   sample    the raw element r is a uint8 when B == 8, else a little-endian uint16; v = min(r, 2^B - 1).  W and H even and >= 16.  Every row and column index,
//             in every image of every stage, is clamped to the image
//   search    s8 = v >> (B - 8) of luma; h = the 2x2 mean of s8, (a + b + c + d + 2) >> 2, W/2 x H/2
//   grid      one vector per 8x8 luma block, nbx = ceil(W / 8), nby = ceil(H / 8).  A vector v = (vx, vy), whole luma samples, is BILATERAL: the block of the
//             picture halfway lies at p - v in C and at p + v in N; the motion from C to N is d = 2v
//   key       l1 = |vx| + |vy|; idx = (vy + R)(2R + 1) + (vx + R); key = cost * 2^15 + l1 * 2^9 + idx; the smallest key wins (cost < 2^16)
//   level 1   R = 8; window: the 8x8 samples of h with origin (4bx - 2, 4by - 2); SAD1(v) = sum |hC[p - v] - hN[p + v]|; cost = SAD1 + 2 l1 -> v1
//   level 0   candidates 2 v1 + delta, delta in [-2, 2]^2 (R = 2 for idx, l1 of the whole vector); window: the 16x16 samples of s8 with origin (8bx - 4, 8by - 4);
//             SAD0(v) = sum |s8C[p - v] - s8N[p + v]|; cost = SAD0 + 4 l1 -> v0, |component| <= 18
//   smoothing per component the median (5th of 9) over the 3x3 block neighbourhood of v0, block indices clamped -> vm
//   fallback  SAD0(vm) + 4 l1(vm) > SAD0(0) ? 0 : vm -> the final field v
//   scene     D = sum over the luma display area of |s8C - s8N|; cut = scene_threshold > 0 && D > scene_threshold * W * H
//   picture   under a cut j becomes 0 if 2j <= f, else f, and all vectors are 0.  Mode blend: all vectors 0, no search, no scene check.
//     offsets   per block and component q = floor((8 d j + f) / (2f)); the C sample lies at 4x - q, the N sample at 4x + (4d - q) in quarter luma samples; chroma:
//               the same numbers in eighths of a chroma sample, 8x - q and 8x + (4d - q)
//     fetch     bilinear, unrounded: luma xi = P >> 2, fx = P & 3, weights (4 - fx)(4 - fy) .. (sum 16); chroma xi = P >> 3, fx = P & 7 (sum 64) -> A (from C), Bn (from N)
//     overlap   luma X = x - 4, i0 = floor(X / 8), ax = X - 8 i0; weights 8 - ax for block i0, ax for block i0 + 1 (clamped), the same vertically (sum 64);
//               chroma X = x - 2, blocks of 4, weights 4 - ax and ax (sum 16)
//     output    num = sum over the four blocks of w ((f - j) A + j Bn); out = (num + 512 f) / (1024 f); num < 2^23
//   margin    as ingest.h: output sample (x, y) outside the display area equals the output sample at (min(x, W - 1), min(y, H - 1))
// k_mcfi_search, one launch per frame pair: a workgroup takes a tile of MC_SB x MC_SB blocks.  Phase 1 stages s8 of C and N, the tile and 24 samples all round
// (level 0 reaches 4 + 18, the half-size image 2 (2 + 8 + 2)), in LDS as bytes, clamped in value, column and row, through deint_run at the planes' alignment class.
// Phase 2 makes the two half-size images out of them (at clamped half-size coordinates) and adds the tile's share of D with the packed byte SAD.  Phase 3, level 1:
// four lanes per block, each takes every fourth vy; per window row it reads seven dwords of either image ONCE and cuts the seventeen horizontal positions out of
// them with v_alignbyte at fixed offsets, seventeen packed SADs side by side.  Phase 4, level 0: the four lanes share the 25 candidates, dynamic offsets, the same
// cut; one of them takes SAD0(0) for the fallback.  Phase 5 writes v0 and the workgroup's part of D.
// k_mcfi_field: sixteen blocks per workgroup, sixteen lanes per block, one per window row: the median of v0, SAD0(vm) from the planes (nothing when vm is 0), the
// fallback; one more workgroup folds the parts of D (an integer sum: any order).
// k_mcfi_render, one launch per output picture: a workgroup takes one tile of MR_TW x MR_TH output samples of one plane, Y first, then Cb, then Cr.  Phase 1 stages
// the tile of C and N with a halo for the largest offset (36 luma samples and one for the fetch; whole runs either side) in LDS as 16-bit samples, clamped, and the
// offsets q and 4d - q of the tile's blocks and their neighbours; it reads D from device memory and decides the cut itself.  Phase 2: a lane takes one run of
// ING_RUN columns of one row; per sample four blocks, two fetches each, all out of LDS.
#pragma once
#include "deint.h"

namespace mihevc {

constexpr int MC_R1 = 8, MC_R0 = 2, MC_VMAX = 2 * MC_R1 + MC_R0;       // search ranges; the largest component of a vector: 18
constexpr int MC_SB = 8;                                              // the search tile: 8 x 8 blocks, four lanes per block
constexpr int MC_SH = 24;                                             // halo of the s8 images
constexpr int MC_SW = 8 * MC_SB + 2 * MC_SH, MC_HW = MC_SW / 2;       // the s8 images: 112 x 112, the half-size ones: 56 x 56
constexpr int MC_HP = 96;                                             // pitch of the half-size images: 24 dwords, so the four lanes of a block, whose rows differ by one,
                                                                      // and the eight blocks of a 32-lane half, one dword apart, read 32 different banks at level 1
constexpr int MC_FB = 16;                                             // blocks per workgroup of k_mcfi_field
constexpr int MR_TW = 64, MR_TH = 32;                                 // the render tile
constexpr int MR_HL = 40, MR_HT = 36;                                 // its luma halo: columns (whole runs), rows
constexpr int MR_LW = MR_TW + 2 * MR_HL, MR_LH = MR_TH + 2 * MR_HT + 1;       // the LDS image of one frame: 144 x 105
constexpr int MR_LP = MR_LW + 2;                                      // its pitch: 73 dwords, so the four rows of a 32-lane half, whose eight runs lie four dwords apart, fall on
                                                                      // 32 different banks when the vectors agree (at 72 dwords: on eight)
constexpr int MR_BW = MR_TW / 4 + 2, MR_BH = MR_TH / 4 + 2;           // blocks a tile's samples weigh (chroma: blocks of 4)
static_assert(MC_SB * MC_SB * 4 == NT && (MR_TW / ING_RUN) * MR_TH == NT && MC_FB * 16 == NT, "lane layouts");

struct McfiSearchShared {
    uint8_t s8[2][MC_SW][MC_SW];        // 25,088 bytes: C, N; row l is row 8 by0 - 24 + l, column i is column 8 bx0 - 24 + i (clamped)
    uint8_t h[2][MC_HW][MC_HP];         // 10,752 bytes: row l is row 4 by0 - 12 + l of the half-size image (clamped)
    uint32_t key1[MC_SB * MC_SB][4], key0[MC_SB * MC_SB][4];
    uint32_t dsum;
};
struct McfiFieldShared {
    uint32_t cell[MC_FB], vm[MC_FB];
    unsigned long long red[NT];
};
struct McfiRenderShared {
    uint16_t f[2][MR_LH][MR_LP];        // 61,320 bytes: C, N; rows begin 4-byte aligned
    int16_t off[MR_BH][MR_BW][4];       // qx, qy, 4dx - qx, 4dy - qy
};

struct McfiSearchArgs {
    const void *cur, *next;             // luma of C and N
    int16_t *v0;                        // nby x nbx x (vx, vy)
    uint32_t *sadz;                     // nby x nbx: SAD0(0)
    unsigned long long *part;           // mcfi_search_workgroups: the parts of D
    int pitch, align, w, h, nbx, nby, shift, vmax;
};
struct McfiFieldArgs {
    const void *cur, *next;
    const int16_t *v0;
    const uint32_t *sadz;
    int16_t *v;
    const unsigned long long *part;
    unsigned long long *dsum;
    int npart, pitch, w, h, nbx, nby, shift, vmax;
};
struct McfiRenderArgs {
    const void *cur[3], *next[3];
    void *dst[3];
    const int16_t *v;                   // the final field (not read under blend)
    const unsigned long long *dsum;     // D (not read when cut_above is 0)
    unsigned long long cut_above;       // scene_threshold * W * H; 0: no scene check
    int pitch[3], dstride[3], align[3];
    int w, h, pw, ph, nbx, nby, vmax, f, j, blend;
};

HDI bool mcfi_geometry_ok(int w, int h) { return w >= 16 && h >= 16 && !(w & 1) && !(h & 1); }
HDI bool mcfi_mode_ok(const mihevc_interpolate *d)
{
    if (!d || d->factor < 2 || d->factor > 4 || (d->mode != 0 && d->mode != 1) || d->scene_threshold < 0 || d->scene_threshold > 255) return false;
    return !(d->reserved[0] | d->reserved[1] | d->reserved[2] | d->reserved[3] | d->reserved[4]);
}
HDI int mcfi_blocks(int n) { return (n + 7) / 8; }
HDI int mcfi_search_workgroups(int w, int h) { return ((mcfi_blocks(w) + MC_SB - 1) / MC_SB) * ((mcfi_blocks(h) + MC_SB - 1) / MC_SB); }
HDI int mcfi_field_workgroups(int w, int h) { return (mcfi_blocks(w) * mcfi_blocks(h) + MC_FB - 1) / MC_FB + 1; }      // the last one folds D
HDI int mcfi_render_tiles(int w, int h) { return ((w + MR_TW - 1) / MR_TW) * ((h + MR_TH - 1) / MR_TH); }
HDI int mcfi_render_workgroups(int pw, int ph) { return mcfi_render_tiles(pw, ph) + 2 * mcfi_render_tiles(pw / 2, ph / 2); }
// every component of the n vectors within the range the render kernel's windows are sized for
inline bool mcfi_vectors_ok(const int16_t *v, size_t n)
{
    for (size_t i = 0; i < 2 * n; i++)
        if (v[i] < -MC_VMAX || v[i] > MC_VMAX) return false;
    return true;
}
// bytes of a session's block: v0, v, SAD0(0), the parts of D and D
struct McfiLayout { size_t v0, v, sadz, part, dsum, bytes; };
inline McfiLayout mcfi_layout(int w, int h)
{
    const size_t nb = (size_t)mcfi_blocks(w) * mcfi_blocks(h);
    McfiLayout l;
    l.part = 0; l.dsum = (size_t)mcfi_search_workgroups(w, h) * 8; l.sadz = l.dsum + 8; l.v0 = l.sadz + nb * 4; l.v = l.v0 + nb * 4; l.bytes = l.v + nb * 4;
    return l;
}
inline McfiSearchArgs mcfi_search_args(int depth, const void *cur, const void *next, int pitch, int w, int h, uint8_t *block)
{
    const McfiLayout l = mcfi_layout(w, h);
    McfiSearchArgs a;
    const size_t pb = (size_t)pitch * (depth > 8 ? 2 : 1);
    const int al0 = ingest_align(cur, pb), al1 = ingest_align(next, pb);
    a.cur = cur; a.next = next; a.v0 = (int16_t *)(block + l.v0); a.sadz = (uint32_t *)(block + l.sadz); a.part = (unsigned long long *)(block + l.part);
    a.pitch = pitch; a.align = al0 < al1 ? al0 : al1; a.w = w; a.h = h; a.nbx = mcfi_blocks(w); a.nby = mcfi_blocks(h); a.shift = depth - 8; a.vmax = (1 << depth) - 1;
    return a;
}
inline McfiFieldArgs mcfi_field_args(const McfiSearchArgs &s, uint8_t *block)
{
    const McfiLayout l = mcfi_layout(s.w, s.h);
    McfiFieldArgs a;
    a.cur = s.cur; a.next = s.next; a.v0 = s.v0; a.sadz = s.sadz; a.v = (int16_t *)(block + l.v); a.part = s.part; a.dsum = (unsigned long long *)(block + l.dsum);
    a.npart = mcfi_search_workgroups(s.w, s.h); a.pitch = s.pitch; a.w = s.w; a.h = s.h; a.nbx = s.nbx; a.nby = s.nby; a.shift = s.shift; a.vmax = s.vmax;
    return a;
}
inline McfiRenderArgs mcfi_render_args(const mihevc_interpolate &m, int j, int depth, const void *const *cur, const void *const *next, int pitch_y, int pitch_c, int w, int h,
                                       int pw, int ph, const int16_t *v, const unsigned long long *dsum, void *const *out, const int *ostride)
{
    McfiRenderArgs a;
    const size_t es = depth > 8 ? 2 : 1;
    for (int c = 0; c < 3; c++) {
        a.cur[c] = cur[c]; a.next[c] = next[c]; a.dst[c] = out[c]; a.dstride[c] = ostride[c]; a.pitch[c] = c ? pitch_c : pitch_y;
        const int al0 = ingest_align(cur[c], (size_t)a.pitch[c] * es), al1 = ingest_align(next[c], (size_t)a.pitch[c] * es);
        a.align[c] = al0 < al1 ? al0 : al1;
    }
    a.v = v; a.dsum = dsum; a.blend = m.mode;
    a.cut_above = m.mode ? 0 : (unsigned long long)m.scene_threshold * (unsigned long long)w * (unsigned long long)h;
    a.w = w; a.h = h; a.pw = pw; a.ph = ph; a.nbx = mcfi_blocks(w); a.nby = mcfi_blocks(h); a.vmax = (1 << depth) - 1; a.f = m.factor; a.j = j;
    return a;
}

DEV uint32_t mcfi_key(int cost, int vx, int vy, int r) { return (uint32_t)cost << 15 | (uint32_t)(iabs(vx) + iabs(vy)) << 9 | (uint32_t)((vy + r) * (2 * r + 1) + vx + r); }
DEV uint32_t umin32(uint32_t a, uint32_t b) { return a < b ? a : b; }
// the level-1 vector of a block out of its four lanes' keys
DEV void mcfi_v1(const uint32_t (&k)[4], int &vx, int &vy)
{
    const int idx = (int)(umin32(umin32(k[0], k[1]), umin32(k[2], k[3])) & 511u);
    vy = idx / (2 * MC_R1 + 1) - MC_R1; vx = idx - (vy + MC_R1) * (2 * MC_R1 + 1) - MC_R1;
}
// SAD0(v) of the block whose window has its origin at (x, y) of the LDS images: C at p - v, N at p + v
DEV int mcfi_sad0(const McfiSearchShared &s, int x, int y, int vx, int vy)
{
    const int oc = x - vx, on = x + vx, bc = oc & ~3, bn = on & ~3, sc = oc & 3, sn = on & 3;
    uint32_t acc = 0;
    for (int r = 0; r < 16; r++) {
        const uint8_t *const pc = &s.s8[0][y - vy + r][bc], *const pn = &s.s8[1][y + vy + r][bn];
        uint32_t c[5], n[5];
#pragma unroll
        for (int k = 0; k < 5; k++) { c[k] = load_u32_aligned(pc + 4 * k); n[k] = load_u32_aligned(pn + 4 * k); }
#pragma unroll
        for (int k = 0; k < 4; k++) acc = sad_packed_u8(align_bytes(c[k + 1], c[k], sc), align_bytes(n[k + 1], n[k], sn), acc);
    }
    return (int)acc;
}

// workgroup `wg` of k_mcfi_search
template <typename T, class Ex> DEV void mcfi_search_program(Ex &ex, McfiSearchShared &s, const McfiSearchArgs &a, int wg)
{
    const int ntx = (a.nbx + MC_SB - 1) / MC_SB;
    if (wg >= mcfi_search_workgroups(a.w, a.h)) return;
    const int ty = wg / ntx, tx = wg - ty * ntx, bx0 = tx * MC_SB, by0 = ty * MC_SB, xl = 8 * bx0 - MC_SH, yl = 8 * by0 - MC_SH;
    const int W = a.w, H = a.h;
    ex.phase([&](int tid) {          // the s8 images: run q % runs of row (q / runs) % MC_SW of frame q / (runs * MC_SW)
        constexpr int runs = MC_SW / ING_RUN;
        if (tid == 0) s.dsum = 0;
        for (int q = tid; q < 2 * MC_SW * runs; q += NT) {
            const int fr = q / (MC_SW * runs), q1 = q - fr * (MC_SW * runs), l = q1 / runs, rn = q1 - l * runs;
            const T *const F = (const T *)(fr ? a.next : a.cur);
            int v[ING_RUN];
            deint_run<T>(F + (ptrdiff_t)clip3(0, H - 1, yl + l) * a.pitch, xl + rn * ING_RUN, W, a.align, a.vmax, v);
#pragma unroll
            for (int k = 0; k < ING_RUN; k++) v[k] >>= a.shift;
            *(ingest_u32x2 *)__builtin_assume_aligned(&s.s8[fr][l][rn * ING_RUN], 8) =
                ingest_u32x2{(uint32_t)v[0] | (uint32_t)v[1] << 8 | (uint32_t)v[2] << 16 | (uint32_t)v[3] << 24,
                             (uint32_t)v[4] | (uint32_t)v[5] << 8 | (uint32_t)v[6] << 16 | (uint32_t)v[7] << 24};
        }
    });
    ex.phase([&](int tid) {          // the half-size images, and the tile's share of D
        for (int q = tid; q < 2 * MC_HW * MC_HW; q += NT) {
            const int fr = q / (MC_HW * MC_HW), q1 = q - fr * (MC_HW * MC_HW), l = q1 / MC_HW, i = q1 - l * MC_HW;
            const int sx = 2 * clip3(0, W / 2 - 1, 4 * bx0 - MC_SH / 2 + i) - xl, sy = 2 * clip3(0, H / 2 - 1, 4 * by0 - MC_SH / 2 + l) - yl;
            s.h[fr][l][i] = (uint8_t)(((int)s.s8[fr][sy][sx] + (int)s.s8[fr][sy][sx + 1] + (int)s.s8[fr][sy + 1][sx] + (int)s.s8[fr][sy + 1][sx + 1] + 2) >> 2);
        }
        const int row = tid >> 2, seg = tid & 3, y = 8 * by0 + row;
        if (y >= H) return;
        uint32_t acc = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int lx = seg * 16 + 4 * k, n = W - (8 * bx0 + lx);
            if (n <= 0) continue;
            const uint32_t m = n >= 4 ? ~0u : (1u << (8 * n)) - 1u;
            acc = sad_packed_u8(load_u32_aligned(&s.s8[0][MC_SH + row][MC_SH + lx]) & m, load_u32_aligned(&s.s8[1][MC_SH + row][MC_SH + lx]) & m, acc);
        }
        if (acc) ex.atomic_add(&s.dsum, acc);
    });
    ex.phase([&](int tid) {          // level 1: lane q of a block takes vy = q - 8, q - 4, ..
        const int lb = tid >> 2, q = tid & 3, lbx = lb & (MC_SB - 1), lby = lb / MC_SB;
        if (bx0 + lbx >= a.nbx || by0 + lby >= a.nby) return;
        const int x = 4 * lbx, y = 4 * lby + MC_SH / 2 - 2;       // the window's origin is column x + 10, row y of the images; the dwords start at column x
        uint32_t best = ~0u;
        for (int vy = q - MC_R1; vy <= MC_R1; vy += 4) {
            uint32_t acc[2 * MC_R1 + 1];
#pragma unroll
            for (int i = 0; i <= 2 * MC_R1; i++) acc[i] = 0;
            for (int r = 0; r < 8; r++) {
                const uint8_t *const pc = &s.h[0][y + r - vy][x], *const pn = &s.h[1][y + r + vy][x];
                uint32_t c[7], n[7];
#pragma unroll
                for (int k = 0; k < 7; k++) { c[k] = load_u32_aligned(pc + 4 * k); n[k] = load_u32_aligned(pn + 4 * k); }
#pragma unroll
                for (int i = 0; i <= 2 * MC_R1; i++) {
                    const int oc = 10 - (i - MC_R1), on = 10 + (i - MC_R1);
#pragma unroll
                    for (int d = 0; d < 2; d++)
                        acc[i] = sad_packed_u8(align_bytes(c[(oc >> 2) + d + 1], c[(oc >> 2) + d], oc & 3), align_bytes(n[(on >> 2) + d + 1], n[(on >> 2) + d], on & 3), acc[i]);
                }
            }
#pragma unroll
            for (int i = 0; i <= 2 * MC_R1; i++) {
                const int vx = i - MC_R1;
                best = umin32(best, mcfi_key((int)acc[i] + 2 * (iabs(vx) + iabs(vy)), vx, vy, MC_R1));
            }
        }
        s.key1[lb][q] = best;
    });
    ex.phase([&](int tid) {          // level 0: lane q takes the candidates q, q + 4, ..; lane 1 SAD0(0) too
        const int lb = tid >> 2, q = tid & 3, lbx = lb & (MC_SB - 1), lby = lb / MC_SB;
        if (bx0 + lbx >= a.nbx || by0 + lby >= a.nby) return;
        const int x = 8 * lbx - 4 + MC_SH, y = 8 * lby - 4 + MC_SH;
        int v1x, v1y;
        mcfi_v1(s.key1[lb], v1x, v1y);
        uint32_t best = ~0u;
        for (int c = q; c < (2 * MC_R0 + 1) * (2 * MC_R0 + 1); c += 4) {
            const int dy = c / (2 * MC_R0 + 1) - MC_R0, dx = c - (dy + MC_R0) * (2 * MC_R0 + 1) - MC_R0, vx = 2 * v1x + dx, vy = 2 * v1y + dy;
            const int l1 = iabs(vx) + iabs(vy);
            best = umin32(best, (uint32_t)(mcfi_sad0(s, x, y, vx, vy) + 4 * l1) << 15 | (uint32_t)l1 << 9 | (uint32_t)c);
        }
        s.key0[lb][q] = best;
        if (q == 1) a.sadz[(size_t)(by0 + lby) * a.nbx + bx0 + lbx] = (uint32_t)mcfi_sad0(s, x, y, 0, 0);
    });
    ex.phase([&](int tid) {
        if (tid == 0) a.part[wg] = s.dsum;
        const int lb = tid >> 2, lbx = lb & (MC_SB - 1), lby = lb / MC_SB;
        if ((tid & 3) || bx0 + lbx >= a.nbx || by0 + lby >= a.nby) return;
        int v1x, v1y;
        mcfi_v1(s.key1[lb], v1x, v1y);
        const int c = (int)(umin32(umin32(s.key0[lb][0], s.key0[lb][1]), umin32(s.key0[lb][2], s.key0[lb][3])) & 511u);
        const int dy = c / (2 * MC_R0 + 1) - MC_R0, dx = c - (dy + MC_R0) * (2 * MC_R0 + 1) - MC_R0;
        store_u32_aligned(a.v0 + 2 * ((size_t)(by0 + lby) * a.nbx + bx0 + lbx), pack_lo16(2 * v1x + dx, 2 * v1y + dy));
    });
}

// the 5th of 9 (a network of 19 exchanges)
DEV int mcfi_median9(int (&p)[9])
{
    auto sw = [&](int i, int j) { const int lo = imin(p[i], p[j]), hi = imax(p[i], p[j]); p[i] = lo; p[j] = hi; };
    sw(1, 2); sw(4, 5); sw(7, 8); sw(0, 1); sw(3, 4); sw(6, 7); sw(1, 2); sw(4, 5); sw(7, 8); sw(0, 3); sw(5, 8); sw(4, 7);
    sw(3, 6); sw(1, 4); sw(2, 5); sw(4, 7); sw(4, 2); sw(6, 4); sw(4, 2);
    return p[4];
}

// workgroup `wg` of k_mcfi_field
template <typename T, class Ex> DEV void mcfi_field_program(Ex &ex, McfiFieldShared &s, const McfiFieldArgs &a, int wg)
{
    const int nb = a.nbx * a.nby, nfw = (nb + MC_FB - 1) / MC_FB;
    if (wg > nfw) return;
    if (wg == nfw) {                 // the fold of D
        ex.phase([&](int tid) {
            unsigned long long acc = 0;
            for (int i = tid; i < a.npart; i += NT) acc += a.part[i];
            s.red[tid] = acc;
        });
        ex.phase([&](int tid) {
            if (tid) return;
            unsigned long long acc = 0;
            for (int i = 0; i < NT; i++) acc += s.red[i];
            *a.dsum = acc;
        });
        return;
    }
    const T *const C = (const T *)a.cur, *const N = (const T *)a.next;
    ex.phase([&](int tid) { if (tid < MC_FB) s.cell[tid] = 0; });
    ex.phase([&](int tid) {          // lane r of a block: the median, and row r of SAD0(vm)
        const int lb = tid >> 4, r = tid & 15, g = wg * MC_FB + lb;
        if (g >= nb) return;
        const int by = g / a.nbx, bx = g - by * a.nbx;
        int px[9], py[9];
#pragma unroll
        for (int k = 0; k < 9; k++) {
            const uint32_t w = load_u32_aligned(a.v0 + 2 * ((size_t)clip3(0, a.nby - 1, by + k / 3 - 1) * a.nbx + clip3(0, a.nbx - 1, bx + k % 3 - 1)));
            px[k] = (int)(int16_t)(w & 0xffffu); py[k] = (int)(int16_t)(w >> 16);
        }
        const int vx = mcfi_median9(px), vy = mcfi_median9(py);
        if (r == 0) s.vm[lb] = pack_lo16(vx, vy);
        if (!(vx | vy)) return;
        const int y = 8 * by - 4 + r, x = 8 * bx - 4;
        const T *const rc = C + (ptrdiff_t)clip3(0, a.h - 1, y - vy) * a.pitch, *const rn = N + (ptrdiff_t)clip3(0, a.h - 1, y + vy) * a.pitch;
        uint32_t acc = 0;
#pragma unroll
        for (int i = 0; i < 16; i++)
            acc += (uint32_t)iabs((imin((int)rc[clip3(0, a.w - 1, x + i - vx)], a.vmax) >> a.shift) - (imin((int)rn[clip3(0, a.w - 1, x + i + vx)], a.vmax) >> a.shift));
        if (acc) ex.atomic_add(&s.cell[lb], acc);
    });
    ex.phase([&](int tid) {
        const int lb = tid >> 4, g = wg * MC_FB + lb;
        if ((tid & 15) || g >= nb) return;
        const uint32_t w = s.vm[lb];
        const int vx = (int)(int16_t)(w & 0xffffu), vy = (int)(int16_t)(w >> 16);
        const bool zero = s.cell[lb] + 4u * (uint32_t)(iabs(vx) + iabs(vy)) > a.sadz[g];
        store_u32_aligned(a.v + 2 * (size_t)g, zero ? 0u : w);
    });
}

// floor((8 d j + f) / (2f)), f in {2, 3, 4}, |8 d j| < 6 * 1024
DEV int mcfi_q(int d, int j, int f)
{
    const int n = 8 * d * j + f;
    return f == 3 ? (int)((uint32_t)(n + 6 * 1024) / 6u) - 1024 : n >> (f == 2 ? 2 : 3);
}
// (num + 512 f) / (1024 f), f in {2, 3, 4}, 0 <= num < 2^23
DEV int mcfi_div(int num, int f)
{
    const int n = (num + 512 * f) >> 10;
    return f == 3 ? (int)(((uint32_t)n * 43691u) >> 17) : n >> (f >> 1);
}

// workgroup r -> component (0 Y, 1 Cb, 2 Cr), r becomes the tile inside it; -1 past the last
HDI int mcfi_render_locate(int pw, int ph, int &r)
{
    const int ny = mcfi_render_tiles(pw, ph), nc = mcfi_render_tiles(pw / 2, ph / 2);
    if (r < ny) return 0;
    r -= ny;
    if (r < nc) return 1;
    r -= nc;
    return r < nc ? 2 : -1;
}

// workgroup `wg` of k_mcfi_render
template <typename T, class Ex> DEV void mcfi_render_program(Ex &ex, McfiRenderShared &s, const McfiRenderArgs &a, int wg)
{
    int tile = wg;
    const int c = mcfi_render_locate(a.pw, a.ph, tile);
    if (c < 0) return;
    T *const dst = (T *)a.dst[c];
    const int pitch = a.pitch[c], dstride = a.dstride[c], al = a.align[c], vmax = a.vmax, f = a.f;
    const int ww = c ? a.w / 2 : a.w, hh = c ? a.h / 2 : a.h, pwo = c ? a.pw / 2 : a.pw, pho = c ? a.ph / 2 : a.ph;
    const int ntx = (pwo + MR_TW - 1) / MR_TW, ty = tile / ntx, tx = tile - ty * ntx, xs = tx * MR_TW, ys = ty * MR_TH;
    const int bl = c ? 2 : 3, pl = c ? 3 : 2;                                // log2 of the block's size in samples of the plane, of the positions' scale
    const int hl = c ? MR_HL / 2 + 4 : MR_HL, ht = c ? MR_HT / 2 : MR_HT;    // halo: whole runs left and right, rows above (one more below)
    const int xl = xs - hl, yl = ys - ht, bxl = (xs >> bl) - 1, byl = (ys >> bl) - 1;
    bool cut = false;
    if (a.cut_above) cut = *a.dsum > a.cut_above;
    const int je = cut ? (2 * a.j <= f ? 0 : f) : a.j;
    const bool still = cut || a.blend;
    ex.phase([&](int tid) {          // the images of C and N, and the offsets of the blocks
        const int runs = (MR_TW + 2 * hl) / ING_RUN, rows = MR_TH + 2 * ht + 1;
        for (int q = tid; q < 2 * rows * runs; q += NT) {
            const int fr = q / (rows * runs), q1 = q - fr * (rows * runs), l = q1 / runs, rn = q1 - l * runs;
            const T *const F = (const T *)(fr ? a.next[c] : a.cur[c]);
            int v[ING_RUN];
            deint_run<T>(F + (ptrdiff_t)clip3(0, hh - 1, yl + l) * pitch, xl + rn * ING_RUN, ww, al, vmax, v);
#pragma unroll
            for (int k = 0; k < ING_RUN; k += 2) store_u32_aligned(&s.f[fr][l][rn * ING_RUN + k], (uint32_t)v[k] | (uint32_t)v[k + 1] << 16);
        }
        for (int q = tid; q < MR_BH * MR_BW; q += NT) {
            const int lj = q / MR_BW, li = q - lj * MR_BW;
            int dx = 0, dy = 0;
            if (!still) {
                const uint32_t w = load_u32_aligned(a.v + 2 * ((size_t)clip3(0, a.nby - 1, byl + lj) * a.nbx + clip3(0, a.nbx - 1, bxl + li)));
                dx = 2 * (int)(int16_t)(w & 0xffffu); dy = 2 * (int)(int16_t)(w >> 16);
            }
            const int qx = mcfi_q(dx, je, f), qy = mcfi_q(dy, je, f);
            s.off[lj][li][0] = (int16_t)qx; s.off[lj][li][1] = (int16_t)qy; s.off[lj][li][2] = (int16_t)(4 * dx - qx); s.off[lj][li][3] = (int16_t)(4 * dy - qy);
        }
    });
    ex.phase([&](int tid) {          // the lane's run of row y
        const int lx = tid & (MR_TW / ING_RUN - 1), ly = tid / (MR_TW / ING_RUN), x0 = xs + lx * ING_RUN, y = ys + ly;
        if (x0 >= pwo || y >= pho) return;
        const int ye = imin(y, hh - 1), bs = 1 << bl, ps = 1 << pl, pm = ps - 1;
        const int Y = ye - bs / 2, j0 = Y >> bl, ay = Y - j0 * bs;
        auto fetch = [&](const uint16_t (&F)[MR_LH][MR_LP], int px, int py) {
            const int xi = (px >> pl) - xl, yi = (py >> pl) - yl, fx = px & pm, fy = py & pm;
            return (ps - fy) * ((ps - fx) * (int)F[yi][xi] + fx * (int)F[yi][xi + 1]) + fy * ((ps - fx) * (int)F[yi + 1][xi] + fx * (int)F[yi + 1][xi + 1]);
        };
        int o[ING_RUN];
#pragma unroll
        for (int k = 0; k < ING_RUN; k++) {
            const int xe = imin(x0 + k, ww - 1), X = xe - bs / 2, i0 = X >> bl, ax = X - i0 * bs;
            int num = 0;
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const int16_t *const e = s.off[j0 - byl + (b >> 1)][i0 - bxl + (b & 1)];
                const int w = ((b & 1) ? ax : bs - ax) * ((b >> 1) ? ay : bs - ay);
                const int A = fetch(s.f[0], ps * xe - e[0], ps * ye - e[1]), Bn = fetch(s.f[1], ps * xe + e[2], ps * ye + e[3]);
                num += w * ((f - je) * A + je * Bn);
            }
            o[k] = mcfi_div(num, f);
        }
        ingest_store(dst + (ptrdiff_t)y * dstride + x0, o, x0 + ING_RUN <= pwo);
    });
}

}  // namespace mihevc
