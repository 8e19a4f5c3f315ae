// hevc_amd/csrc/scale_taps.h — coefficient tables of the polyphase downscaler (kernels/scale.h) and, at the end, of the upscaler
// (kernels/upscale.h): host arithmetic on integers, no HIP
// (tests/emu/scale.cpp exports it to the tests, which hold it against the Fraction tables of tests/scale_ref.py row for row).
//
// One axis of one plane: S source samples become Dn output samples, Dn <= S <= 4 Dn; p = 2: samples centre-aligned, p = 1: output sample 0 co-sited a quarter
// of the way (horizontal chroma, chroma_sample_loc_type 0).  Output sample i sits at pos = ((4i + p) S - p Dn) / (4 Dn) in source index units; its taps are
// the integers k with |pos - k| < 2 S / Dn, weighted CR((pos - k) Dn / S), CR the Catmull-Rom cubic.  With A = (4i + p) S - p Dn and M = 4 S the argument of
// CR is t = (A - 4 Dn k) / M, so with a = |A - 4 Dn k| every weight is an integer over the common denominator 2 M^3:
//   a <= M       2 M^3 CR =  3 a^3 - 5 a^2 M           + 2 M^3
//   M < a < 2 M  2 M^3 CR = -  a^3 + 5 a^2 M - 8 a M^2 + 4 M^3
// c_k = floor(w_k 4096 / sum(w) + 1/2); what the row then lacks to 4096 goes to its largest coefficient (the lowest k among equals); coefficients
// that are 0 at either end of a row are then dropped.  k is NOT clamped here:
// the first index may be negative and first + 15 may pass S - 1; the reader clamps k when it fetches the sample.
#pragma once
#include <cstdint>
#include <vector>

namespace mihevc {

constexpr int SCALE_TAPS = 16;            // coefficients per output sample, zero padded
constexpr int SCALE_ONE = 4096;           // every row sums to this
constexpr int SCALE_MAX_ABS = 6144;       // sum |c_k| of a row: what keeps both passes inside 32 bits

struct ScaleTaps {
    std::vector<int32_t> first;           // per output sample: k of its first coefficient
    std::vector<int16_t> coef;            // per output sample: SCALE_TAPS coefficients from `first` on
    int taps = 0;                         // the longest row: no row has a non-zero coefficient at or past this place
};

inline long long scale_floor_div(long long a, long long b) { return a / b - ((a % b != 0) && ((a < 0) != (b < 0))); }      // b > 0 or b < 0, rounds down

// false: sizes outside the definition, or a row the arithmetic of the kernel has no room for (more than SCALE_TAPS taps, sum |c| above SCALE_MAX_ABS)
inline bool scale_taps_build(int S, int Dn, int p, ScaleTaps &t)
{
    if (S < 1 || Dn < 1 || Dn > S || S > 4 * Dn || S > (1 << 15) || (p != 1 && p != 2)) return false;
    typedef __int128 wide;
    const long long M = 4LL * S, step = 4LL * Dn;
    t.first.assign((size_t)Dn, 0); t.coef.assign((size_t)Dn * SCALE_TAPS, 0); t.taps = 0;
    for (int i = 0; i < Dn; i++) {
        const long long A = (4LL * i + p) * S - (long long)p * Dn;
        // |A - step k| < 2 M
        const long long k0 = scale_floor_div(A - 2 * M, step) + 1, k1 = -scale_floor_div(-(A + 2 * M), step) - 1;
        const int n = (int)(k1 - k0 + 1);
        if (n < 1 || n > SCALE_TAPS) return false;
        wide w[SCALE_TAPS], sum = 0;
        for (int j = 0; j < n; j++) {
            const long long d = A - step * (k0 + j);
            const wide a = d < 0 ? -d : d, m = M;
            w[j] = a <= m ? 3 * a * a * a - 5 * a * a * m + 2 * m * m * m : -(a * a * a) + 5 * a * a * m - 8 * a * m * m + 4 * m * m * m;
            sum += w[j];
        }
        if (sum <= 0) return false;
        int c[SCALE_TAPS], total = 0, best = 0, mag = 0;
        for (int j = 0; j < n; j++) {
            const wide num = 2 * w[j] * SCALE_ONE + sum, den = 2 * sum;
            wide q = num / den;
            if (num % den != 0 && num < 0) q -= 1;
            c[j] = (int)q;
            total += c[j];
            if (c[j] > c[best]) best = j;
        }
        c[best] += SCALE_ONE - total;
        for (int j = 0; j < n; j++) mag += c[j] < 0 ? -c[j] : c[j];
        if (mag > SCALE_MAX_ABS) return false;
        int lead = 0, len = n;      // coefficients that came out 0 at either end of the row are dropped: they read nothing (1:1 is the single tap 4096)
        while (len > 1 && c[lead] == 0) { lead++; len--; }
        while (len > 1 && c[lead + len - 1] == 0) len--;
        t.first[(size_t)i] = (int32_t)(k0 + lead);
        for (int j = 0; j < len; j++) t.coef[(size_t)i * SCALE_TAPS + j] = (int16_t)c[lead + j];
        if (len > t.taps) t.taps = len;
    }
    return true;
}

// The four tables of one source size -> output size pair as the kernel reads them, in one block to upload: 0 luma horizontal, 1 luma vertical, 2 chroma
// horizontal (p = 1), 3 chroma vertical.  first[k] / coef[k]: byte offsets of the int32 first indices and of the int16 coefficient rows (16-byte aligned)
struct ScaleBlock {
    std::vector<uint8_t> bytes;
    size_t first[4], coef[4];
    int taps[4];
};
// tile_h, max_rows: a vertical table must not spread the taps of tile_h adjacent output rows over more than max_rows source rows (the kernel's LDS image)
inline bool scale_block_build(int sw, int sh, int dw, int dh, int tile_h, int max_rows, ScaleBlock &b)
{
    const int S[4] = {sw, sh, sw / 2, sh / 2}, Dn[4] = {dw, dh, dw / 2, dh / 2}, p[4] = {2, 2, 1, 2};
    ScaleTaps t[4];
    size_t total = 0;
    for (int k = 0; k < 4; k++) {
        if (!scale_taps_build(S[k], Dn[k], p[k], t[k])) return false;
        if (k & 1)      // the kernel takes the first index of a tile's first row as the lowest of the tile
            for (int i = 1; i < Dn[k]; i++) if (t[k].first[(size_t)i] < t[k].first[(size_t)i - 1]) return false;
        if (k & 1)
            for (int i = 0; i < Dn[k]; i += tile_h) {
                const int last = i + tile_h - 1 < Dn[k] - 1 ? i + tile_h - 1 : Dn[k] - 1;
                if (t[k].first[(size_t)last] + t[k].taps - t[k].first[(size_t)i] > max_rows) return false;
            }
        b.first[k] = total; total += ((size_t)Dn[k] * sizeof(int32_t) + 15) & ~(size_t)15;
        b.coef[k] = total; total += (size_t)Dn[k] * SCALE_TAPS * sizeof(int16_t);
        b.taps[k] = t[k].taps;
    }
    b.bytes.assign(total, 0);
    for (int k = 0; k < 4; k++) {
        __builtin_memcpy(b.bytes.data() + b.first[k], t[k].first.data(), t[k].first.size() * sizeof(int32_t));
        __builtin_memcpy(b.bytes.data() + b.coef[k], t[k].coef.data(), t[k].coef.size() * sizeof(int16_t));
    }
    return true;
}

// where the four tables of one kind (off: first, coef or near of a block) lie in a copy of the block's bytes at `base`, as T
template <typename T> inline void tap_pointers(const uint8_t *base, const size_t off[4], const T *out[4])
{
    for (int k = 0; k < 4; k++) out[k] = (const T *)(base + off[k]);
}

// ---- the upscaler (kernels/upscale.h): S <= Dn <= 4 S.  The positions are those above; the kernel is NOT stretched, so the taps of output
// sample i are the integers k with |pos - k| < 2 (at most 4) weighted CR(pos - k): with A as above, M = 4 Dn and a = |A - M k| the two polynomials above
// apply over 2 M^3 with this M.  Normalisation and the dropping of end zeros as above (1:1 is the single tap 4096).  near = floor(pos): the anti-ringing clamp
// of the kernel takes the samples at near and near + 1.  Every non-zero coefficient lies in near - 1 .. near + 2, so first - near is in -1 .. 2
constexpr int UPSCALE_TAPS = 4;           // coefficients per output sample, zero padded: rows of 8 bytes
constexpr int UPSCALE_MAX_ABS = 5120;     // sum |c_k| of a row, reached at phase 1/2 ([-256, 2304, 2304, -256])

struct UpscaleTaps {
    std::vector<int32_t> first;           // per output sample: k of its first coefficient
    std::vector<int32_t> near;            // per output sample: floor(pos)
    std::vector<int16_t> coef;            // per output sample: UPSCALE_TAPS coefficients from `first` on
    int taps = 0;                         // the longest row
};

// false: sizes outside the definition, or a row with sum |c| above UPSCALE_MAX_ABS
inline bool scale_taps_build_up(int S, int Dn, int p, UpscaleTaps &t)
{
    if (S < 1 || Dn < S || Dn > 4 * S || Dn > (1 << 15) || (p != 1 && p != 2)) return false;
    typedef __int128 wide;
    const long long M = 4LL * Dn;
    t.first.assign((size_t)Dn, 0); t.near.assign((size_t)Dn, 0); t.coef.assign((size_t)Dn * UPSCALE_TAPS, 0); t.taps = 0;
    for (int i = 0; i < Dn; i++) {
        const long long A = (4LL * i + p) * S - (long long)p * Dn;
        // |A - M k| < 2 M
        const long long k0 = scale_floor_div(A - 2 * M, M) + 1, k1 = -scale_floor_div(-(A + 2 * M), M) - 1, near = scale_floor_div(A, M);
        const int n = (int)(k1 - k0 + 1);
        if (n < 1 || n > UPSCALE_TAPS) return false;
        wide w[UPSCALE_TAPS], sum = 0;
        for (int j = 0; j < n; j++) {
            const long long d = A - M * (k0 + j);
            const wide a = d < 0 ? -d : d, m = M;
            w[j] = a <= m ? 3 * a * a * a - 5 * a * a * m + 2 * m * m * m : -(a * a * a) + 5 * a * a * m - 8 * a * m * m + 4 * m * m * m;
            sum += w[j];
        }
        if (sum <= 0) return false;
        int c[UPSCALE_TAPS], total = 0, best = 0, mag = 0;
        for (int j = 0; j < n; j++) {
            const wide num = 2 * w[j] * SCALE_ONE + sum, den = 2 * sum;
            wide q = num / den;
            if (num % den != 0 && num < 0) q -= 1;
            c[j] = (int)q;
            total += c[j];
            if (c[j] > c[best]) best = j;
        }
        c[best] += SCALE_ONE - total;
        for (int j = 0; j < n; j++) mag += c[j] < 0 ? -c[j] : c[j];
        if (mag > UPSCALE_MAX_ABS) return false;
        int lead = 0, len = n;
        while (len > 1 && c[lead] == 0) { lead++; len--; }
        while (len > 1 && c[lead + len - 1] == 0) len--;
        if (k0 + lead < near - 1 || k0 + lead + len - 1 > near + 2) return false;      // what the kernel's window of four samples rests on
        t.first[(size_t)i] = (int32_t)(k0 + lead);
        t.near[(size_t)i] = (int32_t)near;
        for (int j = 0; j < len; j++) t.coef[(size_t)i * UPSCALE_TAPS + j] = (int16_t)c[lead + j];
        if (len > t.taps) t.taps = len;
    }
    return true;
}

// The four tables of one source size -> output size pair as k_upscale reads them, in one block to upload: 0 luma horizontal, 1 luma vertical, 2 chroma
// horizontal (p = 1), 3 chroma vertical.  first[k] / near[k] / coef[k]: byte offsets of the int32 indices and of the int16 coefficient rows (8-byte aligned)
struct UpscaleBlock {
    std::vector<uint8_t> bytes;
    size_t first[4], near[4], coef[4];
};
// tile_h, halo, max_rows: the kernel's LDS image holds the source rows near - 1 .. near + 2 of tile_h adjacent output rows and of `halo` rows on either side
// of them, max_rows at the most.  The kernel takes near of a tile's first row as the lowest of the tile: near must be monotone.  (`first` need not be and is
// not asked to: at 1:3 the single tap of every third row starts one sample later than the four of the row after it)
inline bool upscale_block_build(int sw, int sh, int dw, int dh, int tile_h, int halo, int max_rows, UpscaleBlock &b)
{
    const int S[4] = {sw, sh, sw / 2, sh / 2}, Dn[4] = {dw, dh, dw / 2, dh / 2}, p[4] = {2, 2, 1, 2};
    UpscaleTaps t[4];
    size_t total = 0;
    for (int k = 0; k < 4; k++) {
        if (!scale_taps_build_up(S[k], Dn[k], p[k], t[k])) return false;
        if (k & 1) {
            for (int i = 1; i < Dn[k]; i++) if (t[k].near[(size_t)i] < t[k].near[(size_t)i - 1]) return false;
            for (int i = 0; i < Dn[k]; i += tile_h) {
                const int lo = i - halo > 0 ? i - halo : 0, hi = i + tile_h - 1 + halo < Dn[k] - 1 ? i + tile_h - 1 + halo : Dn[k] - 1;
                if (t[k].near[(size_t)hi] - t[k].near[(size_t)lo] + 4 > max_rows) return false;
            }
        }
        b.first[k] = total; total += ((size_t)Dn[k] * sizeof(int32_t) + 15) & ~(size_t)15;
        b.near[k] = total; total += ((size_t)Dn[k] * sizeof(int32_t) + 15) & ~(size_t)15;
        b.coef[k] = total; total += ((size_t)Dn[k] * UPSCALE_TAPS * sizeof(int16_t) + 15) & ~(size_t)15;
    }
    b.bytes.assign(total, 0);
    for (int k = 0; k < 4; k++) {
        __builtin_memcpy(b.bytes.data() + b.first[k], t[k].first.data(), t[k].first.size() * sizeof(int32_t));
        __builtin_memcpy(b.bytes.data() + b.near[k], t[k].near.data(), t[k].near.size() * sizeof(int32_t));
        __builtin_memcpy(b.bytes.data() + b.coef[k], t[k].coef.data(), t[k].coef.size() * sizeof(int16_t));
    }
    return true;
}

}  // namespace mihevc
