// hevc_amd/csrc/kernels/fieldmatch.h — inverse telecine (mihevc_send_frame_fieldmatch, mihevc_k_fieldmatch_metrics, mihevc_k_fieldmatch_weave): woven frames
// F_k of the session's display size, planar 4:2:0 at the session's own depth B (8 or 10), whose fields are matched back into the film frames they were made of.
// Integers only, so that the device, the stepped kernels (tests/emu/fieldmatch.cpp) and the numpy model (tests/fieldmatch_ref.py) agree bit for bit.  The
// definition (normative: DESIGN.md §6h; the plan that reads the metrics is csrc/fieldmatch_plan.h):
//   sample      the raw element r is a uint8 when B == 8, else a little-endian uint16; v = min(r, 2^B - 1)
//   geometry    W even, H a multiple of 4, both >= 16 (deint_geometry_ok)
//   keep        parity of the rows of the declared first field (tff ? 0 : 1).  For frame k: P = F_(k-1) (the first frame: itself), C = F_k, N = F_(k+1) (the
//               last frame: itself)
//   candidates  W_m, m in {c, p, n}: rows of parity keep from C, the other rows from X_c = C, X_p = P, X_n = N; the same weave in Y, Cb and Cr
//   comb        luma, signed ints, T = 9 << (B - 8), for 1 <= y <= H - 2 and 0 <= x < W:
//                 d1 = W_m[y-1][x] - W_m[y][x]        d2 = W_m[y+1][x] - W_m[y][x]
//                 combed: (d1 > T && d2 > T) || (d1 < -T && d2 < -T); strength min(|d1|, |d2|), 0 when not combed
//               S_m = sum of the strengths; K_m = the largest number of combed samples in any 16 x 16 block of the grid anchored at (0, 0) (partial blocks count
//               what they have)
//   duplicate   luma, rows of parity keep only: q = |C[y][x] - P[y][x]|; DS = sum of q; DB = the largest sum of q over any block of 32 columns x 32 frame rows
//               (16 kept rows) of the grid anchored at (0, 0).  (The clip's first frame: both all-ones, set by the caller of the kernel.)
//   picture     W_match in all three planes, values clamped; margin as ingest.h: output sample (x, y) outside the display area equals the output sample at
//               (min(x, W - 1), min(y, H - 1))
// k_fm_metrics, one launch per frame: a workgroup takes one luma tile of FM_TW x FM_TH samples (multiples of 32: no block straddles tiles).  Phase 1 stages the
// tile's rows and one above and below of C, of P (its kept rows inside the tile for the duplicate metrics, its other rows for W_p) and the other rows of N in LDS
// as 16-bit samples, clamped in value: every source row of a tile is read from memory once per workgroup, through deint_run (ingest_load at the planes'
// alignment class; a run that reaches past W reads its elements one by one at clamped columns, and those samples are not counted).  No access is wider than the
// planes' alignment and none lies outside the caller's rows: a plane may end with its last sample.  Phase 2 clears the block cells.  Phase 3: a lane takes one
// run of ING_RUN columns of one pair of rows, reads four rows of each candidate from LDS and adds its counts, strengths and differences to the cells of its
// blocks with integer LDS atomics (16 lanes per comb block, 64 per duplicate block).  Phase 4: four lanes fold the cells into the workgroup's eight partials
// (S_c S_p S_n K_c K_p K_n DS DB) and store them at part[wg].  k_fm_fold, one workgroup, folds the partials of all workgroups (sums, and maxima for the K and
// DB) into out[8]: nothing has to be zeroed in front, and integer sums and maxima do not depend on the order they are taken in.
// k_fm_weave, one launch per picture: the deinterlacer's tile order (deint_locate) and lanes, no LDS: a lane copies its run of a pair of rows, the kept row from
// C and the other from X_match, through deint_run and ingest_store.
#pragma once
#include "deint.h"

namespace mihevc {

constexpr int FM_TW = 128, FM_TH = 32;                        // the metrics tile in luma samples
constexpr int FM_RUNS = FM_TW / ING_RUN, FM_LH = FM_TH + 2;   // runs per row and rows of an LDS image
constexpr int FM_CB = (FM_TW / 16) * (FM_TH / 16);            // comb blocks (16 x 16) of a tile
constexpr int FM_DB = FM_TW / 32;                             // duplicate blocks (32 x 32) of a tile (FM_TH == 32: one row of them)
constexpr int FM_COMB_T = 9;                                  // the threshold T at 8 bit
static_assert(FM_TH == 32 && FM_TW % 32 == 0 && FM_RUNS * (FM_TH / 2) == NT, "one lane per run of a row pair; one row of duplicate blocks");

struct FmShared {
    uint16_t f[3][FM_LH][FM_TW];       // 0 C, 1 P, 2 N; 26,112 bytes; row l is row ty * FM_TH - 1 + l of the plane, column i is column tx * FM_TW + i
    uint32_t k[3][FM_CB], s[3][FM_CB]; // combed samples and strengths per comb block
    uint32_t dq[FM_DB];                // sums of q per duplicate block
    uint64_t red[NT / 8][8];           // k_fm_fold: the lanes' partial folds
};

struct FmArgs {
    const void *prev, *cur, *next;     // luma of P, C and N (they may be the same plane)
    unsigned long long *part;          // fm_workgroups(w, h) x 8
    int pitch, align;                  // of every frame, in elements; the narrowest class of the three (ingest_align)
    int w, h, keep, vmax, thr;
};

HDI bool fieldmatch_mode_ok(const mihevc_fieldmatch *d)
{
    if (!d || (d->tff != 0 && d->tff != 1) || (d->decimate != 0 && d->decimate != 1) || (d->deint != 0 && d->deint != 1)) return false;
    return !(d->reserved[0] | d->reserved[1] | d->reserved[2] | d->reserved[3] | d->reserved[4]);
}
HDI int fm_workgroups(int w, int h) { return ((w + FM_TW - 1) / FM_TW) * ((h + FM_TH - 1) / FM_TH); }
inline FmArgs fm_args(int depth, const void *prev, const void *cur, const void *next, int pitch, int w, int h, int keep, unsigned long long *part)
{
    FmArgs a;
    const size_t pb = (size_t)pitch * (depth > 8 ? 2 : 1);
    const int al0 = ingest_align(prev, pb), al1 = ingest_align(cur, pb), al2 = ingest_align(next, pb);
    a.prev = prev; a.cur = cur; a.next = next; a.part = part; a.pitch = pitch;
    a.align = al0 < al1 ? (al0 < al2 ? al0 : al2) : (al1 < al2 ? al1 : al2);
    a.w = w; a.h = h; a.keep = keep; a.vmax = (1 << depth) - 1; a.thr = FM_COMB_T << (depth - 8);
    return a;
}

// the combed samples of one row and their strengths: up / mid / dn are W_m[y-1], W_m[y], W_m[y+1] at the lane's columns, nv of them inside the picture
DEV void fm_comb_row(const int (&up)[ING_RUN], const int (&mid)[ING_RUN], const int (&dn)[ING_RUN], int nv, int thr, uint32_t &count, uint32_t &strength)
{
#pragma unroll
    for (int k = 0; k < ING_RUN; k++) {
        const int d1 = up[k] - mid[k], d2 = dn[k] - mid[k];
        const bool combed = k < nv && ((d1 > thr && d2 > thr) || (d1 < -thr && d2 < -thr));
        count += combed ? 1u : 0u;
        strength += combed ? (uint32_t)imin(iabs(d1), iabs(d2)) : 0u;
    }
}

// workgroup `wg` of k_fm_metrics
template <typename T, class Ex> DEV void fm_metrics_program(Ex &ex, FmShared &s, const FmArgs &a, int wg)
{
    const int ntx = (a.w + FM_TW - 1) / FM_TW, ty = wg / ntx, tx = wg - ty * ntx;
    if (wg >= fm_workgroups(a.w, a.h)) return;
    const T *const F[3] = {(const T *)a.cur, (const T *)a.prev, (const T *)a.next};
    const int W = a.w, H = a.h, keep = a.keep, yl = ty * FM_TH - 1, xl = tx * FM_TW;
    ex.phase([&](int tid) {          // the images: run q % FM_RUNS of row (q / FM_RUNS) % FM_LH of image q / (FM_RUNS * FM_LH)
        for (int q = tid; q < 3 * FM_LH * FM_RUNS; q += NT) {
            const int img = q / (FM_LH * FM_RUNS), rq = q - img * (FM_LH * FM_RUNS), l = rq / FM_RUNS, rn = rq - l * FM_RUNS, x0 = xl + rn * ING_RUN, r = yl + l;
            if (x0 >= W || r < 0 || r >= H) continue;
            const bool kept = (r & 1) == keep, inside = l >= 1 && l <= FM_TH;
            if (img == 1 && kept && !inside) continue;       // P's kept rows serve the duplicate metrics of the tile's own rows only
            if (img == 2 && kept) continue;                  // N gives W_n its other rows, nothing else
            int v[ING_RUN];
            deint_run<T>(F[img] + (ptrdiff_t)r * a.pitch, x0, W, a.align, a.vmax, v);
            *(ingest_u32x4 *)__builtin_assume_aligned(&s.f[img][l][rn * ING_RUN], 16) =
                ingest_u32x4{(uint32_t)v[0] | (uint32_t)v[1] << 16, (uint32_t)v[2] | (uint32_t)v[3] << 16, (uint32_t)v[4] | (uint32_t)v[5] << 16, (uint32_t)v[6] | (uint32_t)v[7] << 16};
        }
    });
    ex.phase([&](int tid) {
        if (tid < 3 * FM_CB) { (&s.k[0][0])[tid] = 0; (&s.s[0][0])[tid] = 0; }
        if (tid < FM_DB) s.dq[tid] = 0;
    });
    ex.phase([&](int tid) {          // the lane's run of rows ya and ya + 1 (ya even)
        const int lx = tid & (FM_RUNS - 1), ly = tid / FM_RUNS, x0 = xl + lx * ING_RUN, ya = ty * FM_TH + 2 * ly;
        if (x0 >= W || ya >= H) return;                      // (H is even: row ya + 1 is inside when ya is)
        const int nv = imin(ING_RUN, W - x0), l = 2 * ly + 1, col = lx * ING_RUN, cb = (ly / 8) * (FM_TW / 16) + lx / 2;
        const bool row_a = ya >= 1, row_b = ya + 1 <= H - 2;  // the rows whose comb is taken
        for (int m = 0; m < 3; m++) {
            int r[4][ING_RUN];                               // W_m at rows ya - 1, ya, ya + 1, ya + 2: the kept ones from C, the others from X_m
#pragma unroll
            for (int i = 0; i < 4; i++) deint_lds_run(&s.f[((ya + 1 + i) & 1) == keep ? 0 : m][l - 1 + i][col], r[i]);
            uint32_t cnt = 0, str = 0;
            if (row_a) fm_comb_row(r[0], r[1], r[2], nv, a.thr, cnt, str);
            if (row_b) fm_comb_row(r[1], r[2], r[3], nv, a.thr, cnt, str);
            if (cnt) { ex.atomic_add(&s.k[m][cb], cnt); ex.atomic_add(&s.s[m][cb], str); }
        }
        int c[ING_RUN], p[ING_RUN];
        const int lk = l + (keep ? 1 : 0);                   // the pair's kept row
        deint_lds_run(&s.f[0][lk][col], c);
        deint_lds_run(&s.f[1][lk][col], p);
        uint32_t q = 0;
#pragma unroll
        for (int k = 0; k < ING_RUN; k++) q += k < nv ? (uint32_t)iabs(c[k] - p[k]) : 0u;
        if (q) ex.atomic_add(&s.dq[lx / 4], q);
    });
    ex.phase([&](int tid) {
        if (tid < 3) {
            unsigned long long sum = 0, top = 0;
            for (int b = 0; b < FM_CB; b++) { sum += s.s[tid][b]; top = s.k[tid][b] > top ? s.k[tid][b] : top; }
            a.part[(size_t)wg * 8 + tid] = sum; a.part[(size_t)wg * 8 + 3 + tid] = top;
        } else if (tid == 3) {
            unsigned long long sum = 0, top = 0;
            for (int b = 0; b < FM_DB; b++) { sum += s.dq[b]; top = s.dq[b] > top ? s.dq[b] : top; }
            a.part[(size_t)wg * 8 + 6] = sum; a.part[(size_t)wg * 8 + 7] = top;
        }
    });
}

// k_fm_fold's one workgroup: out[j] = the sum (j < 3, j == 6) or the maximum of part[i * 8 + j] over the n workgroups of k_fm_metrics
template <class Ex> DEV void fm_fold_program(Ex &ex, FmShared &s, const unsigned long long *part, int n, unsigned long long *out)
{
    auto is_sum = [](int j) { return j < 3 || j == 6; };
    ex.phase([&](int tid) {
        const int j = tid & 7;
        unsigned long long acc = 0;
        for (int i = tid >> 3; i < n; i += NT / 8) {
            const unsigned long long v = part[(size_t)i * 8 + j];
            acc = is_sum(j) ? acc + v : v > acc ? v : acc;
        }
        s.red[tid >> 3][j] = acc;
    });
    ex.phase([&](int tid) {
        if (tid >= 8) return;
        unsigned long long acc = 0;
        for (int i = 0; i < NT / 8; i++) acc = is_sum(tid) ? acc + s.red[i][tid] : s.red[i][tid] > acc ? s.red[i][tid] : acc;
        out[tid] = acc;
    });
}

// workgroup `wg` of k_fm_weave.  a: deint_args with cur = C and prev = X_match (next and second are not read)
template <typename T, class Ex> DEV void fm_weave_program(Ex &ex, const DeintArgs &a, int wg)
{
    int tile = wg;
    const int c = deint_locate(a.pw, a.ph, tile);
    if (c < 0) return;
    const T *const C = (const T *)a.cur[c], *const X = (const T *)a.prev[c];
    T *const dst = (T *)a.dst[c];
    const int ww = c ? a.w / 2 : a.w, hh = c ? a.h / 2 : a.h, pwo = c ? a.pw / 2 : a.pw, pho = c ? a.ph / 2 : a.ph;
    const int ntx = (pwo + DI_TW - 1) / DI_TW, ty = tile / ntx, tx = tile - ty * ntx;
    ex.phase([&](int tid) {
        const int lx = tid & (DI_LX - 1), ly = tid / DI_LX, x0 = tx * DI_TW + lx * ING_RUN;
        if (x0 >= pwo) return;
        for (int i = 0; i < 2; i++) {
            const int y = ty * DI_TH + 2 * ly + i;
            if (y >= pho) return;
            const int ye = imin(y, hh - 1);
            int o[ING_RUN];
            deint_run<T>(((ye & 1) == a.keep ? C : X) + (ptrdiff_t)ye * a.pitch[c], x0, ww, a.align[c], a.vmax, o);      // (past W: the last sample inside)
            ingest_store(dst + (ptrdiff_t)y * a.dstride[c] + x0, o, x0 + ING_RUN <= pwo);
        }
    });
}

}  // namespace mihevc
