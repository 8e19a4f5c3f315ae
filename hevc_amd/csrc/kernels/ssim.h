// hevc_amd/csrc/kernels/ssim.h — per-picture SSIM (cfg.ssim; x265 --ssim) of the source against the final reconstruction over the CODED size, per colour
// component.  The textbook SSIM (Wang et al.) on 8x8 windows at stride 4 with biased variances, stated in integers up to one division per window so that the
// device, the stepped kernel and the numpy reference (tests/ssim_ref.py) agree bit for bit and nothing depends on scheduling:
//   blocks   4x4 samples on the 4-sample grid (coded plane sizes are multiples of 4: they tile every plane), a = source, b = reconstruction:
//            s1 = sum a, s2 = sum b, ss = sum (a^2 + b^2), s12 = sum a b
//   windows  2x2 adjacent blocks (8x8 samples), (W/4 - 1)(H/4 - 1) per plane; a window's sums are its four blocks' sums
//   in int64 vars = 64 ss - s1^2 - s2^2, covar = 64 s12 - s1 s2, c1 = (4096 peak^2 + 5000) / 10000, c2 = (9 * 4096 peak^2 + 5000) / 10000 ((0.01 peak)^2 and
//            (0.03 peak)^2 scaled by 64^2, rounded), f1 = 2 s1 s2 + c1, f2 = 2 covar + c2, g1 = s1^2 + s2^2 + c1, g2 = vars + c2: all below 2^53, exact as doubles
//   q        (double(f1) * double(f2)) / (double(g1) * double(g2)): three correctly rounded IEEE operations; Q = rint(q * 2^32) (ties to even) as int64.
//            q lies in (-1, 1]: anti-correlated windows are negative and stay so
//   picture  the int64 sum of Q over the windows; SSIM = sum / (windows * 2^32) is formed on the host
// Two launches per step, each covering every picture of the batch and all three components (the shape of kernels/pichash.h):
//   k_ssim       one workgroup per region of SSIM_RW x SSIM_RH windows: phase 1 — one lane per 4x4 block of the region plus one block column / row of halo
//                (a dword per row and picture at 8 bit, two at 16 bit; lanes side by side take blocks side by side) leaves the block's sums in LDS; phase 2 —
//                one lane per window adds four blocks and forms Q; the workgroup reduces Q in int64 to one partial.  The halo blocks are recomputed, not
//                exchanged: no workgroup depends on another
//   k_ssim_fold  one workgroup per (picture, component): the partials -> one int64.  No atomics on global memory, nothing to zero in front, no
//                floating-point sum: integer sums are order-independent
#pragma once
#include "common.h"

namespace mihevc {

constexpr int SSIM_RW = 32, SSIM_RH = 8;                    // windows per workgroup: one per lane
constexpr int SSIM_BW = SSIM_RW + 1, SSIM_BH = SSIM_RH + 1; // blocks it needs
constexpr int SSIM_NB = SSIM_BW * SSIM_BH;
static_assert(SSIM_RW * SSIM_RH == NT, "one window per lane");

template <int BD> struct SsimConst {
    static constexpr long long peak = (1ll << BD) - 1;
    static constexpr long long c1 = (4096 * peak * peak + 5000) / 10000, c2 = (9 * 4096 * peak * peak + 5000) / 10000;
    // a window holds 64 samples of each picture: s1, s2 <= 64 peak, ss <= 128 peak^2, s12 <= 64 peak^2; so s1^2 + s2^2 and 64 ss <= 8192 peak^2, and
    // |f1|, |f2|, g1, g2 <= 8192 peak^2 + c2: every int64 product is exact and the conversions to double are too
    static_assert(8192 * peak * peak + c2 < (1ll << 53), "window terms must stay below 2^53");
    static_assert(128 * peak * peak < (1ll << 32) && 64 * peak < (1ll << 16), "block and window sums are kept in 32 bits, s1 | s2 << 16 per block");
};

// one component of one picture pair: w x h samples, strides in samples
template <typename T> struct SsimPlane {
    const T *a, *b;
    int stride_a, stride_b, w, h;
};
HDI int ssim_windows_x(int w) { return w / 4 - 1; }
HDI int ssim_windows_y(int h) { return h / 4 - 1; }
HDI int ssim_regions_x(int w) { return (ssim_windows_x(w) + SSIM_RW - 1) / SSIM_RW; }
HDI int ssim_regions(int w, int h) { return ssim_regions_x(w) * ((ssim_windows_y(h) + SSIM_RH - 1) / SSIM_RH); }
// The workgroups of a picture cover Y, then Cb, then Cr (nr_y / nr_c regions each).  workgroup r -> component, r becomes the region inside it; -1 past the last
HDI int ssim_locate(int nr_y, int nr_c, int &r)
{
    if (r < nr_y) return 0;
    r -= nr_y;
    if (r < 2 * nr_c) { const int c = 1 + r / nr_c; r -= (c - 1) * nr_c; return c; }
    return -1;
}
HDI int ssim_first_region(int nr_y, int nr_c, int c) { return c ? nr_y + (c - 1) * nr_c : 0; }

struct SsimShared {
    uint32_t s[SSIM_NB];        // s1 | s2 << 16
    uint32_t ss[SSIM_NB];
    uint32_t s12[SSIM_NB];
    long long red[NT];
};

// four samples side by side
DEV void ssim_load4(const uint8_t *p, int (&v)[4])
{
    const uint32_t d = load_u32(p);
#pragma unroll
    for (int k = 0; k < 4; k++) v[k] = (int)((d >> (8 * k)) & 255u);
}
DEV void ssim_load4(const uint16_t *p, int (&v)[4])
{
    const uint32_t d0 = load_u32(p), d1 = load_u32(p + 2);
    v[0] = (int)(d0 & 0xffffu); v[1] = (int)(d0 >> 16); v[2] = (int)(d1 & 0xffffu); v[3] = (int)(d1 >> 16);
}

// Q of one window from its sums (steps 3 and 4 of the definition)
template <int BD> DEV long long ssim_window_q32(uint32_t s1, uint32_t s2, uint32_t ss, uint32_t s12)
{
    const long long a = s1, b = s2, c1 = SsimConst<BD>::c1, c2 = SsimConst<BD>::c2;
    const long long sq = a * a + b * b, vars = 64ll * (long long)ss - sq, covar = 64ll * (long long)s12 - a * b;
    const long long f1 = 2 * a * b + c1, f2 = 2 * covar + c2, g1 = sq + c1, g2 = vars + c2;
    const double q = ((double)f1 * (double)f2) / ((double)g1 * (double)g2);
    return (long long)__builtin_rint(q * 4294967296.0);
}

// 256 int64 -> red[0]: four per lane of the first wave, then halving steps inside that wave
template <class Ex> DEV void ssim_reduce(Ex &ex, SsimShared &s)
{
    ex.wave_step([&](int tid) {
        if (tid < 64) s.red[tid] = s.red[tid] + s.red[tid + 64] + s.red[tid + 128] + s.red[tid + 192];
    });
    for (int h = 32; h > 0; h >>= 1)
        ex.wave_step([&](int tid) {
            if (tid < h) s.red[tid] += s.red[tid + h];
        });
}

// region `reg` of component q: the sum of Q over its windows -> *part
template <typename T, class Ex> DEV void ssim_region_program(Ex &ex, SsimShared &s, const SsimPlane<T> &q, int reg, long long *part)
{
    constexpr int BD = PixTraits<T>::kBitDepth;
    const int nrx = ssim_regions_x(q.w), ry = reg / nrx, rx = reg - ry * nrx;
    const int bx0 = rx * SSIM_RW, by0 = ry * SSIM_RH, nbx = q.w / 4, nby = q.h / 4;      // the region's first block; blocks of the plane
    ex.phase([&](int tid) {
        for (int i = tid; i < SSIM_NB; i += NT) {
            const int ly = i / SSIM_BW, lx = i - ly * SSIM_BW, bx = bx0 + lx, by = by0 + ly;
            if (bx >= nbx || by >= nby) continue;      // past the plane: no window of the picture reads this block
            const T *pa = q.a + (ptrdiff_t)(4 * by) * q.stride_a + 4 * bx, *pb = q.b + (ptrdiff_t)(4 * by) * q.stride_b + 4 * bx;
            int va[4][4], vb[4][4];
#pragma unroll
            for (int r = 0; r < 4; r++) { ssim_load4(pa + (ptrdiff_t)r * q.stride_a, va[r]); ssim_load4(pb + (ptrdiff_t)r * q.stride_b, vb[r]); }
            uint32_t s1 = 0, s2 = 0, ss = 0, s12 = 0;
#pragma unroll
            for (int r = 0; r < 4; r++)
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const uint32_t x = (uint32_t)va[r][k], y = (uint32_t)vb[r][k];
                    s1 += x; s2 += y; ss += x * x + y * y; s12 += x * y;
                }
            s.s[i] = s1 | (s2 << 16); s.ss[i] = ss; s.s12[i] = s12;
        }
    });
    ex.phase([&](int tid) {
        const int ly = tid / SSIM_RW, lx = tid - ly * SSIM_RW;
        long long v = 0;
        if (bx0 + lx < nbx - 1 && by0 + ly < nby - 1) {
            const int i = ly * SSIM_BW + lx;
            const uint32_t p = s.s[i], p1 = s.s[i + 1], p2 = s.s[i + SSIM_BW], p3 = s.s[i + SSIM_BW + 1];
            const uint32_t s1 = (p & 0xffffu) + (p1 & 0xffffu) + (p2 & 0xffffu) + (p3 & 0xffffu), s2 = (p >> 16) + (p1 >> 16) + (p2 >> 16) + (p3 >> 16);
            v = ssim_window_q32<BD>(s1, s2, s.ss[i] + s.ss[i + 1] + s.ss[i + SSIM_BW] + s.ss[i + SSIM_BW + 1],
                                    s.s12[i] + s.s12[i + 1] + s.s12[i + SSIM_BW] + s.s12[i + SSIM_BW + 1]);
        }
        s.red[tid] = v;
    });
    ssim_reduce(ex, s);
    ex.wave_step([&](int tid) { if (tid == 0) *part = s.red[0]; });
}

// a component's nr partials -> *out
template <class Ex> DEV void ssim_fold_program(Ex &ex, SsimShared &s, int nr, const long long *part, long long *out)
{
    ex.phase([&](int tid) {
        long long acc = 0;
        for (int r = tid; r < nr; r += NT) acc += part[r];
        s.red[tid] = acc;
    });
    ssim_reduce(ex, s);
    ex.wave_step([&](int tid) { if (tid == 0) *out = s.red[0]; });
}

}  // namespace mihevc
