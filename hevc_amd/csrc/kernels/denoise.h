// hevc_amd/csrc/kernels/denoise.h — denoising source (mihevc_send_frame_denoise, mihevc_k_denoise): three progressive frames P (previous), C (current), N (next),
// planar 4:2:0 at the session's own depth B (8 or 10) -> the filtered picture of C in the session's planes, margin included.  A motion-adaptive spatio-temporal
// filter: a weighted mean of the sample, its eight neighbours in C and the co-sited samples of P and N, every weight a threshold minus a difference, so edges,
// impulses and moving areas pass unfiltered.  Integers only, so that the device, the stepped kernel (tests/emu/denoise.cpp) and the numpy model
// (tests/denoise_ref.py) agree bit for bit.  The definition (normative: DESIGN.md §6g):
//   sample    the raw element r is a uint8 when B == 8, else a little-endian uint16; v = min(r, 2^B - 1)
//   strengths luma_spatial, luma_temporal, chroma_spatial, chroma_temporal in 8-bit units, 0 .. 255; for a plane Ts = spatial << (B - 8), Tt = temporal << (B - 8):
//             Y takes the luma pair, Cb and Cr the chroma pair
//   geometry  the plane is Wp x Hp (luma W x H, both even and >= 16; chroma W/2 x H/2); column indices are clamped to [0, Wp - 1], row indices to [0, Hp - 1], in
//             all three frames
//   D_F[q]    |F[q] - C[q]| for F in {P, N}
//   centre    wc = max(Ts, Tt, 1)
//   spatial   for the 8 neighbours q of p in the 3x3 window of C: ws(q) = max(0, Ts - |C[q] - C[p]|)
//   temporal  for F in {P, N}: m_F = (sum over the 3x3 window of k(q) D_F[q] + 8) >> 4, k = (1 2 1; 2 4 2; 1 2 1); d_F = max(D_F[p], m_F); wt_F = max(0, Tt - d_F)
//   output    W = wc + sum ws(q) + wt_P + wt_N; acc = wc C[p] + sum ws(q) C[q] + wt_P P[p] + wt_N N[p]; out = (acc + (W >> 1)) / W, integer division.
//             W <= 11 * 1020 and acc + W / 2 < 2^24; out is a weighted mean of samples: no clamp
//   margin    as ingest.h: output sample (x, y) outside the display area equals the output sample at (min(x, W - 1), min(y, H - 1))
// One launch per output picture (k_denoise): a workgroup takes one tile of DN_TW x DN_TH output samples of one plane, the tiles of Y first, then Cb, then Cr: the
// deinterlacer's tile, so its tile count and deint_locate serve here.  Phase 1 stages the tile's rows of C, P and N, one more above and below and one run either
// side (one column is needed; a whole run keeps the image's runs on the plane's runs), in LDS as 16-bit samples, clamped in value, column and row: deint_run,
// that is ingest_load at the planes' alignment class inside the plane and single elements at clamped columns across its edge.  No access is wider than the
// planes' alignment and none lies outside the caller's rows.  Phase 2: a lane takes one run of ING_RUN columns of two rows.  Per image row it reads the run and
// its two neighbours of each frame (one 16-byte and two 2-byte LDS reads) and makes the horizontal 1-2-1 pass over D_P and D_N ONCE, both sums side by side in
// one 32-bit word (each <= 4 * 1023); four rows serve the lane's two output rows, and the vertical pass adds three such words.  The division is a multiplication
// by the fp32 reciprocal and one correction step either way: the numerator is exact in fp32 and the quotient at most 1023, so the product is off by far less
// than 1 and the corrected quotient is exact whatever the last bit of the reciprocal.
#pragma once
#include "deint.h"

namespace mihevc {

constexpr int DN_TW = DI_TW, DN_TH = DI_TH;                       // the tile: 128 x 32 output samples, 16 runs side by side x 16 row pairs
constexpr int DN_LW = DN_TW + 2 * ING_RUN, DN_LH = DN_TH + 2;     // the LDS image of one frame: 144 x 34
constexpr int DN_RUNS = DN_LW / ING_RUN;

struct DenoiseShared {
    uint16_t f[3][DN_LH][DN_LW];    // 29,376 bytes: C, P, N; row l is row ty * DN_TH - 1 + l of the plane, column i is column tx * DN_TW - ING_RUN + i
};

struct DenoiseArgs {
    DeintArgs f;                    // the three frames, the output planes and the geometry (keep and second unused)
    int ts[3], tt[3];               // per plane: the thresholds at the planes' depth
};

HDI bool denoise_geometry_ok(int w, int h) { return w >= 16 && h >= 16 && !(w & 1) && !(h & 1); }
HDI bool denoise_strength_ok(const mihevc_denoise *d)
{
    if (!d) return false;
    if ((d->luma_spatial | d->luma_temporal | d->chroma_spatial | d->chroma_temporal) & ~255) return false;
    return !(d->reserved[0] | d->reserved[1] | d->reserved[2] | d->reserved[3]);
}
// every field from the strengths, the geometry and the planes (as deint_args)
inline DenoiseArgs denoise_args(const mihevc_denoise &d, int depth, const void *const *prev, const void *const *cur, const void *const *next, int pitch_y, int pitch_c,
                                int w, int h, int pw, int ph, void *const *out, const int *ostride)
{
    DenoiseArgs a;
    a.f = deint_args(depth, prev, cur, next, pitch_y, pitch_c, w, h, pw, ph, 0, 0, out, ostride);
    for (int c = 0; c < 3; c++) {
        a.ts[c] = (c ? d.chroma_spatial : d.luma_spatial) << (depth - 8);
        a.tt[c] = (c ? d.chroma_temporal : d.luma_temporal) << (depth - 8);
    }
    return a;
}

// n / w for 0 <= n < 2^24, w >= 1, n / w < 2^12
DEV int denoise_div(int n, int w)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const float rc = __builtin_amdgcn_rcpf((float)w);
#else
    const float rc = 1.0f / (float)w;
#endif
    const int q = (int)((float)n * rc), r = n - q * w;
    return q + (r >= w) - (r < 0);
}

// one image row of the lane: C at columns x0 - 1 .. x0 + ING_RUN, and the horizontal 1-2-1 sums of D_P (low half) and D_N (high half) at x0 .. x0 + ING_RUN - 1
struct DenoiseRow {
    int c[ING_RUN + 2];
    uint32_t h[ING_RUN];
};
// ING_RUN + 2 samples around the run at p (16-byte aligned)
DEV void denoise_lds_run(const uint16_t *p, int (&v)[ING_RUN + 2])
{
    deint_lds_run(p, v + 1);
    v[0] = (int)p[-1];
    v[ING_RUN + 1] = (int)p[ING_RUN];
}
DEV void denoise_row(const DenoiseShared &s, int l, int col, DenoiseRow &r)
{
    int p[ING_RUN + 2], n[ING_RUN + 2];
    uint32_t d[ING_RUN + 2];
    denoise_lds_run(&s.f[0][l][col], r.c);
    denoise_lds_run(&s.f[1][l][col], p);
    denoise_lds_run(&s.f[2][l][col], n);
#pragma unroll
    for (int k = 0; k < ING_RUN + 2; k++) d[k] = (uint32_t)iabs(p[k] - r.c[k]) | (uint32_t)iabs(n[k] - r.c[k]) << 16;
#pragma unroll
    for (int k = 0; k < ING_RUN; k++) r.h[k] = d[k] + 2 * d[k + 1] + d[k + 2];
}
// the output row whose window is the rows up, mid, dn; pc / nc: P and N at the run's own columns of the middle row
DEV void denoise_filter(const DenoiseRow &up, const DenoiseRow &mid, const DenoiseRow &dn, const int (&pc)[ING_RUN], const int (&nc)[ING_RUN], int ts, int tt,
                        int (&o)[ING_RUN])
{
    const int wc = imax(imax(ts, tt), 1);
#pragma unroll
    for (int k = 0; k < ING_RUN; k++) {
        const int c = mid.c[k + 1];
        int W = wc, acc = wc * c;
        auto spatial = [&](int q) { const int w = imax(0, ts - iabs(q - c)); W += w; acc += w * q; };
#pragma unroll
        for (int j = 0; j < 3; j++) { spatial(up.c[k + j]); spatial(dn.c[k + j]); }
        spatial(mid.c[k]); spatial(mid.c[k + 2]);
        const uint32_t m = up.h[k] + 2 * mid.h[k] + dn.h[k] + 0x00080008u;
        const int wp = imax(0, tt - imax(iabs(pc[k] - c), (int)(m & 0xffffu) >> 4)), wn = imax(0, tt - imax(iabs(nc[k] - c), (int)(m >> 20)));
        W += wp + wn; acc += wp * pc[k] + wn * nc[k];
        o[k] = denoise_div(acc + (W >> 1), W);
    }
}

// workgroup `wg` of the launch
template <typename T, class Ex> DEV void denoise_tile_program(Ex &ex, DenoiseShared &s, const DenoiseArgs &a, int wg)
{
    int tile = wg;
    const int c = deint_locate(a.f.pw, a.f.ph, tile);
    if (c < 0) return;
    T *const dst = (T *)a.f.dst[c];
    const int pitch = a.f.pitch[c], dstride = a.f.dstride[c], al = a.f.align[c], vmax = a.f.vmax, ts = a.ts[c], tt = a.tt[c];
    const int ww = c ? a.f.w / 2 : a.f.w, hh = c ? a.f.h / 2 : a.f.h, pwo = c ? a.f.pw / 2 : a.f.pw, pho = c ? a.f.ph / 2 : a.f.ph;
    const int ntx = (pwo + DN_TW - 1) / DN_TW, ty = tile / ntx, tx = tile - ty * ntx;
    const int xl = tx * DN_TW - ING_RUN, yl = ty * DN_TH - 1;            // column and row of the images' first sample
    ex.phase([&](int tid) {          // the images of C, P and N: run q % DN_RUNS of row (q / DN_RUNS) % DN_LH of frame q / (DN_RUNS * DN_LH)
        for (int q = tid; q < 3 * DN_LH * DN_RUNS; q += NT) {
            const int fr = q / (DN_LH * DN_RUNS), q1 = q - fr * (DN_LH * DN_RUNS), l = q1 / DN_RUNS, rn = q1 - l * DN_RUNS, x0 = xl + rn * ING_RUN, r = yl + l;
            if (x0 >= pwo + ING_RUN || r > hh) continue;                 // no lane of phase 2 reads it
            const T *const F = (const T *)(fr == 0 ? a.f.cur[c] : fr == 1 ? a.f.prev[c] : a.f.next[c]);
            int v[ING_RUN];
            deint_run<T>(F + (ptrdiff_t)clip3(0, hh - 1, r) * pitch, x0, ww, al, vmax, v);
            *(ingest_u32x4 *)__builtin_assume_aligned(&s.f[fr][l][rn * ING_RUN], 16) =
                ingest_u32x4{(uint32_t)v[0] | (uint32_t)v[1] << 16, (uint32_t)v[2] | (uint32_t)v[3] << 16, (uint32_t)v[4] | (uint32_t)v[5] << 16, (uint32_t)v[6] | (uint32_t)v[7] << 16};
        }
    });
    ex.phase([&](int tid) {          // the lane's run of rows y and y + 1
        const int lx = tid & (DI_LX - 1), ly = tid / DI_LX, x0 = tx * DN_TW + lx * ING_RUN, y = ty * DN_TH + 2 * ly, col = (lx + 1) * ING_RUN;
        if (x0 >= pwo || y >= pho) return;                               // (coded heights are multiples of 4 at least: y + 1 < pho with y)
        const int last = ww - 1 - x0;                                    // the run's last sample inside the display area (>= 0)
        const int ye = imin(y, hh - 1), l = ye - yl;                     // the image row of the first output row; a row of the margin repeats row hh - 1
        const bool two = y + 1 < hh;                                     // the second output row is a row of its own
        DenoiseRow r0, r1, r2;
        int pc[ING_RUN], nc[ING_RUN], o[ING_RUN];
        denoise_row(s, l - 1, col, r0);
        denoise_row(s, l, col, r1);
        denoise_row(s, l + 1, col, r2);
        deint_lds_run(&s.f[1][l][col], pc);
        deint_lds_run(&s.f[2][l][col], nc);
        denoise_filter(r0, r1, r2, pc, nc, ts, tt, o);
#pragma unroll
        for (int k = 1; k < ING_RUN; k++) o[k] = k > last ? o[k - 1] : o[k];          // the margin's columns repeat the last one inside
        ingest_store(dst + (ptrdiff_t)y * dstride + x0, o, x0 + ING_RUN <= pwo);
        if (two) {
            denoise_row(s, l + 2, col, r0);
            deint_lds_run(&s.f[1][l + 1][col], pc);
            deint_lds_run(&s.f[2][l + 1][col], nc);
            denoise_filter(r1, r2, r0, pc, nc, ts, tt, o);
#pragma unroll
            for (int k = 1; k < ING_RUN; k++) o[k] = k > last ? o[k - 1] : o[k];
        }
        ingest_store(dst + (ptrdiff_t)(y + 1) * dstride + x0, o, x0 + ING_RUN <= pwo);
    });
}

}  // namespace mihevc
