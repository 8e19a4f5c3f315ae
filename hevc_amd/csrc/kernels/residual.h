// hevc_amd/csrc/kernels/residual.h — K3: forward transform, quantisation, scaling, inverse transform and
// reconstruction of all transform units of one CTU, executed by the CTU's workgroup on its LDS image.
//
// Index space: the CTU image of ctu_image.h (1536 samples: luma, Cb, Cr).  The TU a sample belongs to is
// looked up in `tu_log2[16]` (CU size per 8x8 luma tile, 0 = no TU there); chroma TUs are the co-located half-size
// blocks.  Arithmetic: H.265 8.6.2-8.6.4 (scaling, transformation) for the decoder side; the conventional
// two-stage integer forward transform and dead-zone quantiser for the encoder side — identical, term for term, to
// oracle/hevc_oracle.c (orc_fwd_transform, orc_quant, orc_dequant, orc_inv_transform).
// Roofline note: 4 matrix passes of <=32 MACs per sample; the working set never leaves LDS (12 KiB per CTU).
#pragma once
#include "common.h"
#include "ctu_image.h"

namespace mihevc {

// pair tables: offsets of the 4-, 8-, 16-, 32-point sections (n/2 x n dwords each)
DEV int pair_off(int log2n) { return log2n == 2 ? 0 : log2n == 3 ? 8 : log2n == 4 ? 40 : 168; }

struct ResidualShared {
    // transform matrices as dword pairs for v_dot2_i32_i16, laid out so that the lanes of a wave (consecutive x)
    // read consecutive dwords: mp[off + p*n + u] = (M[u][2p], M[u][2p+1]),  mq[off + p*n + y] = (M[2p][y], M[2p+1][y])
    alignas(16) uint32_t mp[680];
    alignas(16) uint32_t mq[680];
    union {
    struct {
    alignas(16) int16_t res[1536];         // residual in, reconstructed residual out
    alignas(16) int16_t tmp[1536];         // stage intermediates, row-pair interleaved: element (r, c) at (r & ~1) * stride + 2c + (r & 1)
    alignas(16) int16_t coef[1536];        // transform coefficients / inverse stage-1 output (natural layout)
    alignas(16) int16_t lvl[1536];         // quantised levels (TU-local raster at CTU coordinates)
    uint32_t desc[1536];       // TU geometry (pack_loc), indexed by sample but DEFINED ONLY AT THE ORIGIN OF EACH 2x4 BLOCK of the caller's region (Region::block_index):
                               // the entries residual_pipeline reads.  The caller writes them (fill_desc, or its own loop over the blocks) while it forms the residual
    };
    alignas(16) uint32_t scratch[4608];    // the same 18 KB for a caller's own use while no residual is in flight (k_inter_ctu: fractional search)
    struct { alignas(16) int16_t res_[1536]; int sb_bits[CTU_SUBBLOCKS]; } post;      // over `tmp`, which is idle once the inverse transform is done: a caller's level bits per 4x4 sub-block (k_inter_ctu: RD zero-out, then the rate estimate)
    struct { alignas(16) long long d[192]; int b[192]; } cg;      // over `res`, which is idle between the forward and the inverse transform: per 2x4 block, its share of a coefficient group's distortion and bits
    };
    uint8_t tu_log2[16];       // per 8x8 luma tile: log2 of the TU (= CU) size, 0 = none
    uint8_t tu_intra[16];      // per tile: 1 = intra rounding
    unsigned cbf[3];           // bit t set: tile t's TU has a non-zero level in that plane (all tiles of a TU set the TU's first tile bit)
    int quant_scale[6], level_scale[6];   // LDS copies: no global-memory read on the per-sample path
};

struct SampleLoc : CtuSample {      // where the sample is in the CTU image, and the TU that holds it
    int log2n, tx0, ty0;       // TU geometry in the same coordinates; log2n == 0: not covered
    int tile0;                 // 8x8 tile index of the TU origin (for the cbf word)
    int intra;
    int scan;                  // scanIdx of the TU (7.4.9.11): 0 diagonal, 1 horizontal, 2 vertical; locate() leaves it 0, intra callers set it
};

// A square luma region of the CTU (cx, cy, size 2^log2n) plus its two co-located chroma blocks: 1.5 n^2 samples.
// Phases that only concern one CU enumerate the region instead of all 1536 CTU samples.
struct Region {
    int cx, cy, log2n;
    DEV int count() const { return (1 << (2 * log2n)) + (1 << (2 * log2n - 1)); }
    // k-th block of (1 << lh) rows x (1 << lw) columns of the region (luma first, then Cb, Cr) -> index of its top-left sample in the CTU image
    DEV int at(int k, int lw, int lh) const
    {
        const int nb = 1 << (2 * log2n - lw - lh);             // luma blocks
        if (k < nb) { const int per = log2n - lw; return ctu_index(0, cx + ((k & ((1 << per) - 1)) << lw), cy + ((k >> per) << lh)); }
        k -= nb;
        const int q = nb >> 2, pl = k >= q, kk = pl ? k - q : k, per = log2n - 1 - lw;
        return ctu_index(1 + pl, (cx >> 1) + ((kk & ((1 << per) - 1)) << lw), (cy >> 1) + ((kk >> per) << lh));
    }
    DEV int index(int k) const { return at(k, 0, 0); }              // k-th sample of count()
    DEV int block_index(int k) const { return at(k, 2, 1); }        // k-th block of 2 rows x 4 columns, count() / 8 of them
};
DEV Region whole_ctu() { return Region{0, 0, 5}; }

DEV SampleLoc locate(const ResidualShared &s, int idx)
{
    SampleLoc l;
    static_cast<CtuSample &>(l) = ctu_sample(idx);
    int sh = l.plane ? 2 : 3;                       // samples per tile edge: 8 luma, 4 chroma
    int tile = (l.y >> sh) * 4 + (l.x >> sh);
    int lg = s.tu_log2[tile];
    l.intra = s.tu_intra[tile];
    l.scan = 0;
    if (!lg) { l.log2n = 0; l.tx0 = l.ty0 = l.tile0 = 0; return l; }
    int lgp = l.plane ? lg - 1 : lg;
    l.log2n = lgp;
    l.tx0 = l.x & ~((1 << lgp) - 1);
    l.ty0 = l.y & ~((1 << lgp) - 1);
    l.tile0 = (l.ty0 >> sh) * 4 + (l.tx0 >> sh);
    return l;
}
// packed form kept in LDS so the five transform phases do one read instead of re-deriving the geometry
DEV uint32_t pack_loc(const SampleLoc &l) { return (uint32_t)l.log2n | (uint32_t)l.tx0 << 3 | (uint32_t)l.ty0 << 8 | (uint32_t)l.tile0 << 13 | (uint32_t)l.intra << 17 | (uint32_t)l.scan << 18; }
DEV SampleLoc unpack_loc(uint32_t d, int idx)
{
    SampleLoc l;
    static_cast<CtuSample &>(l) = ctu_sample(idx);
    l.log2n = (int)(d & 7); l.tx0 = (int)(d >> 3) & 31; l.ty0 = (int)(d >> 8) & 31; l.tile0 = (int)(d >> 13) & 15; l.intra = (int)(d >> 17) & 1; l.scan = (int)(d >> 18) & 3;
    return l;
}

// the descriptors residual_pipeline reads for region rg: one per 2x4 block, at the block's origin, each written by one lane.  scan(l): the TU's scanIdx
template <class Scan> DEV void fill_desc(ResidualShared &s, Region rg, int tid, Scan &&scan)
{
    for (int k = tid; k < (rg.count() >> 3); k += NT) {
        const int idx = rg.block_index(k);
        SampleLoc l = locate(s, idx);
        l.scan = scan(l);
        s.desc[idx] = pack_loc(l);
    }
}

// 16 / 8 bytes of an LDS image whose address is 16- / 8-byte aligned as one ds_read_b128 / ds_read_b64 (and the matching stores)
DEV void load_x4(const void *p, uint32_t (&v)[4]) { __builtin_memcpy(v, __builtin_assume_aligned(p, 16), 16); }
DEV void load_x2(const void *p, uint32_t (&v)[2]) { __builtin_memcpy(v, __builtin_assume_aligned(p, 8), 8); }
DEV void store_x4(void *p, const uint32_t (&v)[4]) { __builtin_memcpy(__builtin_assume_aligned(p, 16), v, 16); }
DEV void store_x2(void *p, const uint32_t (&v)[2]) { __builtin_memcpy(__builtin_assume_aligned(p, 8), v, 8); }
// four horizontally adjacent entries of a CTU image (p 4-entry aligned) as the 16-bit pairs (e0, e1), (e2, e3) the packed helpers of common.h work on
DEV void load4_pk(const uint8_t *p, uint32_t (&v)[2])
{
    const uint32_t d = load_u32_aligned(p);
    v[0] = perm_bytes(0u, d, 0x04010400u); v[1] = perm_bytes(0u, d, 0x04030402u);      // (selector 4: a zero byte)
}
DEV void load4_pk(const uint16_t *p, uint32_t (&v)[2]) { load_x2(p, v); }
DEV void load4_pk(const int16_t *p, uint32_t (&v)[2]) { load_x2(p, v); }

// scanIdx of a TU (7.4.9.11): mode-dependent for intra 4x4 TUs and 8x8 luma TUs, diagonal otherwise
DEV int scan_idx_of(int log2n, int c_idx, int mode)
{
    if (log2n == 2 || (log2n == 3 && c_idx == 0)) {
        if (mode >= 6 && mode <= 14) return 2;
        if (mode >= 22 && mode <= 30) return 1;
    }
    return 0;
}
// raster position (y * 4 + x) of scan position n inside a 4x4 group (6.5.3 up-right diagonal, 6.5.4 horizontal, 6.5.5 vertical)
constexpr int scan4_pos(int scan, int n) { return scan == 1 ? n : scan == 2 ? ((n & 3) << 2) | (n >> 2) : (int)((0xFBE7AD369C258140ull >> (4 * n)) & 15); }

// The encoder's quantiser for one TU (flat m = 16): dead-zone quantisation with rounding offset 171/512 (intra) or 85/512 (inter),
// and scaling (8.6.4.1).  qp is the syntax QP; the two tables (quant_scale, level_scale) are the caller's LDS copies.
struct Quantiser {
    int qs, qbits, bd_shift;
    long long add, scale;
    template <typename TQ, typename TL>
    DEV Quantiser(int qp, int bit_depth, int log2n, int intra, const TQ *qs_tab, const TL *ls_tab)
    {
        const int q = qp + 6 * (bit_depth - 8);
        qs = qs_tab[q % 6];
        qbits = 14 + q / 6 + (15 - bit_depth - log2n);
        bd_shift = bit_depth + log2n - 5;
        add = (long long)(intra ? 171 : 85) << (qbits - 9);
        scale = (long long)16 * ls_tab[q % 6] << (q / 6);
    }
    DEV int level(int c) const        // signed level, |level| clipped to 32767
    {
        const long long a = ((long long)iabs(c) * qs + add) >> qbits, m = a > 32767 ? 32767 : a;
        return (int)(c < 0 ? -m : m);
    }
    DEV int dequant(int lv) const     // scaled level, clipped to 16 bit (|lv| <= 32767 and QP <= 51 keep the shifted product below 2^28)
    {
        return clip3(-32768, 32767, (int)((lv * scale + ((long long)1 << (bd_shift - 1))) >> bd_shift));
    }
};

// Sign data hiding, encoder side (7.3.8.11 signHidden: the decoder infers the sign of the group's first level from the parity of its
// absolute sum when lastSigScanPos - firstSigScanPos > 3).  One 4x4 group after quantisation by qz: lv[16] levels and c[16] forward coefficients
// in raster order.  When the parity disagrees with the first level's sign, the one +-1 change whose rounding
// error costs least is made (cost of scan position n: -delta for +1, delta for -1, delta = (|c| qs - |L| << qbits) >> (qbits - 8); ties
// to the highest n; the first level may not drop to 0; a new level before the first one must carry the first one's sign; never above the
// last level, so which TUs and groups hold levels does not change).  Returns the raster position of the changed level and its new value in
// `nv`, or -1 when nothing changes.  SCAN is a template argument so that every index is a constant: the arrays stay in registers.
template <int SCAN> DEV int sdh_adjust(const int (&lv)[16], const int (&c)[16], const Quantiser &qz, int &nv)
{
    int first = 16, last = -1, sum = 0;
#pragma unroll
    for (int n = 0; n < 16; n++) {
        const int v = lv[scan4_pos(SCAN, n)];
        if (v) { first = first < 16 ? first : n; last = n; sum += iabs(v); }
    }
    if (last - first <= 3) return -1;
    int sf = 0;
#pragma unroll
    for (int n = 0; n < 16; n++) if (n == first) sf = lv[scan4_pos(SCAN, n)] < 0;
    if ((sum & 1) == sf) return -1;
    long long best = 0;
    int bp = -1;
#pragma unroll
    for (int n = 15; n >= 0; n--) {
        const int p = scan4_pos(SCAN, n), a = iabs(lv[p]);
        if (n > last) continue;
        const long long u = (long long)iabs(c[p]) * qz.qs, delta = (u - ((long long)a << qz.qbits)) >> (qz.qbits - 8);
        int chg;
        long long cost;
        if (a) {
            if (delta > 0) { chg = 1; cost = -delta; }
            else { if (n == first && a == 1) continue; chg = -1; cost = delta; }
        } else {
            if (n < first && (c[p] < 0) != (sf != 0)) continue;
            chg = 1; cost = -delta;
        }
        if (bp < 0 || cost < best) {
            best = cost; bp = p;
            const int na = chg > 0 && a == 32767 ? a - 1 : a + chg;
            nv = c[p] < 0 ? -na : na;
        }
    }
    return bp;
}
DEV int sdh_adjust_scan(int scan, const int (&lv)[16], const int (&c)[16], const Quantiser &qz, int &nv)
{
    return scan == 1 ? sdh_adjust<1>(lv, c, qz, nv) : scan == 2 ? sdh_adjust<2>(lv, c, qz, nv) : sdh_adjust<0>(lv, c, qz, nv);
}

// ------------------------------------------------------------------------------------------ 4x4 core
// One 4x4 TU (4-point DCT, or DST-VII for intra luma) with one lane per sample: the per-lane steps of the NxN trial (intra.h intra_cu_nxn)
// and of k_transform4_blocks (transform4_program).  M is the 4x4 matrix [k * 4 + n]; i the lane's sample (y * 4 + x).  Each caller runs the
// steps in this order, every step in a wave step or phase of its own: fwd_rows, fwd_cols_quant, (sign_hide, one lane per block,) inv_cols, inv_rows.
struct Block4 {
    int16_t res[16];          // residual in; the forward coefficients after fwd_cols_quant when sign hiding wants them (the residual is spent)
    int16_t lvl[16];          // levels
    int tmp[16];              // stage intermediates
    unsigned nz;              // 1: the block has a non-zero level (the caller zeroes it before fwd_cols_quant)
};
DEV void core4_fwd_rows(const int16_t *M, Block4 &b, int i, int bit_depth)
{
    const int u = i & 3, y = i >> 2, s1 = bit_depth - 7;
    int acc = 0;
#pragma unroll
    for (int x = 0; x < 4; x++) acc += M[u * 4 + x] * b.res[y * 4 + x];
    b.tmp[i] = (acc + (1 << (s1 - 1))) >> s1;
}
template <class Ex> DEV void core4_fwd_cols_quant(Ex &ex, const int16_t *M, Block4 &b, int i, const Quantiser &qz, bool keep_coef)
{
    const int u = i & 3, v = i >> 2;
    int acc = 0;
#pragma unroll
    for (int y = 0; y < 4; y++) acc += M[v * 4 + y] * b.tmp[y * 4 + u];
    const int c = clip3(-32768, 32767, (acc + 128) >> 8), lv = qz.level(c);
    b.lvl[i] = (int16_t)lv;
    if (keep_coef) b.res[i] = (int16_t)c;
    if (lv) ex.atomic_or(&b.nz, 1u);
}
DEV void core4_sign_hide(Block4 &b, int scan, const Quantiser &qz)      // a 4x4 TU is one coefficient group
{
    int lv[16], c[16], nv = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) { lv[j] = b.lvl[j]; c[j] = b.res[j]; }
    const int p = sdh_adjust_scan(scan, lv, c, qz, nv);
    if (p >= 0) b.lvl[p] = (int16_t)nv;
}
DEV void core4_inv_cols(const int16_t *M, Block4 &b, int i, const Quantiser &qz)      // scaling + inverse stage 1, 16-bit clip
{
    if (!b.nz) return;
    const int x = i & 3, y = i >> 2;
    int acc = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) acc += M[j * 4 + y] * qz.dequant(b.lvl[j * 4 + x]);
    b.tmp[i] = clip3(-32768, 32767, (acc + 64) >> 7);
}
DEV int core4_inv_rows(const int16_t *M, const Block4 &b, int i, int bit_depth)      // -> the lane's reconstructed residual
{
    if (!b.nz) return 0;
    const int x = i & 3, y = i >> 2, s3 = 20 - bit_depth;
    int acc = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) acc += M[j * 4 + x] * b.tmp[y * 4 + j];
    return (int)(int16_t)((acc + (1 << (s3 - 1))) >> s3);
}

// forward + quant + scaling + inverse for every TU of the region; s.desc must describe the region's samples
// (callers fill it while they form the residual).  qp / qp_c are syntax QPs.
// One lane owns a BLOCK of 2 rows x 4 columns of outputs per stage (TUs are at least 4x4 and 4-aligned, so a block never straddles a
// TU): a matrix operand fetched once (ds_read_b128 / b64) feeds 8 v_dot2_i32_i16, the sample operands come as b128 rows or as the
// row-pair dwords of `tmp`, results leave as b64 / b128 stores.  The one-output-per-lane form spent two ds_read_b32 per dot2 and was
// LDS-issue bound (a third of k_inter_ctu's instructions, profiles/r02 phase table); a CTU is 192 blocks = one pass of the workgroup.
// cg_lam_q4 > 0 (inter CTUs): RD zero-out of 4x4 coefficient groups, oracle cg_zero_out — dropping a group adds D = sum r (2c - r) of squared
// coefficient error (c coefficient, r its reconstruction) and saves its levels' bits + one sub-block; drop <=> 16 D < ((cg_lam_q4 * bits) >> 4) << 2 (15 - bitDepth - log2n).
// A group is two vertically adjacent 2x4 blocks, i.e. two lanes: both leave their partial sums in LDS (`res` is free between the forward and the
// inverse transform) and the next phase lets each decide for its own half.
// sign_hide: after the group decisions, every 4x4 group is brought to the sign data hiding parity (sdh_adjust) by the lane of its upper
// 2x4 block; the TU's scanIdx comes with s.desc.  Skipped by a uniform branch when off.
template <class Ex> DEV void residual_pipeline(Ex &ex, ResidualShared &s, int qp, int qp_c, int bit_depth, Region rg, int cg_lam_q4 = 0, int sign_hide = 0)
{
    const int nblk = rg.count() >> 3;
    constexpr int kZero[2][4] = {};
    long long *cg_d = s.cg.d;
    int *cg_b = s.cg.b;
    // row stages (forward 1, inverse 2): out(y, u) = sum_p M-pair(p, u) . in(y, 2p..2p+1); column stages (forward 2, inverse 1):
    // out(v, x) = sum_p M-pair(p, v) . in-row-pair(p, x), the row pairs of `tmp` being single dwords.  Both add to the caller's zeroed `acc`;
    // round8 then rounds, shifts and clips the block's eight sums
    auto round8 = [](int (&v)[2][4], auto &&f) {
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int i = 0; i < 4; i++) v[j][i] = f(v[j][i]);
    };
    auto row_stage = [&](const uint32_t *mat, const int16_t *in, const SampleLoc &l, int (&acc)[2][4]) {
        const int n = 1 << l.log2n, u4 = l.x - l.tx0;
        const uint32_t *m = mat + pair_off(l.log2n) + u4;
        const int16_t *r0 = in + l.base + l.y * l.stride + l.tx0, *r1 = r0 + l.stride;
        if (n == 4) {
            uint32_t d0[2], d1[2];
            load_x2(r0, d0); load_x2(r1, d1);
#pragma unroll
            for (int p = 0; p < 2; p++) {
                uint32_t mm[4];
                load_x4(m + p * 4, mm);
#pragma unroll
                for (int i = 0; i < 4; i++) { acc[0][i] = dot2_i16(mm[i], d0[p], acc[0][i]); acc[1][i] = dot2_i16(mm[i], d1[p], acc[1][i]); }
            }
            return;
        }
        for (int p0 = 0; p0 < n / 2; p0 += 4) {
            uint32_t d0[4], d1[4];
            load_x4(r0 + 2 * p0, d0); load_x4(r1 + 2 * p0, d1);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                uint32_t mm[4];
                load_x4(m + (p0 + j) * n, mm);
#pragma unroll
                for (int i = 0; i < 4; i++) { acc[0][i] = dot2_i16(mm[i], d0[j], acc[0][i]); acc[1][i] = dot2_i16(mm[i], d1[j], acc[1][i]); }
            }
        }
    };
    auto col_stage = [&](const uint32_t *mat, const SampleLoc &l, int (&acc)[2][4]) {
        const int n = 1 << l.log2n, v2 = l.y - l.ty0;
        const uint32_t *m = mat + pair_off(l.log2n) + v2;
        const int16_t *t = s.tmp + l.base + l.ty0 * l.stride + 2 * l.x;
#pragma unroll 4
        for (int p = 0; p < n / 2; p++) {
            uint32_t d[4], mm[2];
            load_x4(t + 2 * p * l.stride, d);
            load_x2(m + p * n, mm);
#pragma unroll
            for (int i = 0; i < 4; i++) { acc[0][i] = dot2_i16(mm[0], d[i], acc[0][i]); acc[1][i] = dot2_i16(mm[1], d[i], acc[1][i]); }
        }
    };
    // rows (y, y+1) x columns (x..x+3) into the row-pair interleaved `tmp`: four dwords
    auto store_pairs = [&](const SampleLoc &l, const int (&v)[2][4]) {
        uint32_t o[4];
#pragma unroll
        for (int i = 0; i < 4; i++) o[i] = pack_lo16(v[0][i], v[1][i]);
        store_x4(s.tmp + l.base + l.y * l.stride + 2 * l.x, o);
    };
    auto store_rows = [&](int16_t *dst, const SampleLoc &l, const int (&v)[2][4]) {
#pragma unroll
        for (int j = 0; j < 2; j++) {
            uint32_t o[2] = {pack_lo16(v[j][0], v[j][1]), pack_lo16(v[j][2], v[j][3])};
            store_x2(dst + l.base + (l.y + j) * l.stride + l.x, o);
        }
    };
    ex.phase([&](int tid) {      // forward stage 1: rows
        for (int k = tid; k < nblk; k += NT) {
            const int idx = rg.block_index(k);
            SampleLoc l = unpack_loc(s.desc[idx], idx);
            if (!l.log2n) continue;
            const int sh1 = l.log2n + bit_depth - 9;
            int acc[2][4] = {};
            row_stage(s.mp, s.res, l, acc);
            round8(acc, [&](int v) { return sh1 > 0 ? (v + (1 << (sh1 - 1))) >> sh1 : v; });
            store_pairs(l, acc);
        }
    });
    ex.phase([&](int tid) {      // forward stage 2: columns
        for (int k = tid; k < nblk; k += NT) {
            const int idx = rg.block_index(k);
            SampleLoc l = unpack_loc(s.desc[idx], idx);
            if (!l.log2n) continue;
            const int sh2 = l.log2n + 6;
            int acc[2][4] = {};
            col_stage(s.mp, l, acc);
            round8(acc, [&](int v) { return clip3(-32768, 32767, (v + (1 << (sh2 - 1))) >> sh2); });
            store_rows(s.coef, l, acc);
        }
    });
    ex.phase([&](int tid) {      // quantisation + scaling (8.6.4.1, flat m = 16)
        for (int k = tid; k < nblk; k += NT) {
            const int idx = rg.block_index(k);
            SampleLoc l = unpack_loc(s.desc[idx], idx);
            int lev[2][4], deq[2][4];
            if (!l.log2n) { store_rows(s.lvl, l, kZero); continue; }
            const Quantiser qz(l.plane ? qp_c : qp, bit_depth, l.log2n, l.intra, s.quant_scale, s.level_scale);
            const bool cg = cg_lam_q4 > 0 && !l.intra;
            int any = 0, bits = 0;
            long long dsum = 0;
#pragma unroll
            for (int j = 0; j < 2; j++) {
                uint32_t c2[2];
                load_x2(s.coef + l.base + (l.y + j) * l.stride + l.x, c2);
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int c = (int)(int16_t)(c2[i >> 1] >> (16 * (i & 1)));
                    const int lv = qz.level(c);
                    lev[j][i] = lv;
                    any |= lv;
                    deq[j][i] = qz.dequant(lv);
                    if (cg && lv) { bits += rate_level(iabs(lv)); dsum += (long long)deq[j][i] * (2 * c - deq[j][i]); }
                }
            }
            store_rows(s.lvl, l, lev);
            store_pairs(l, deq);
            if (cg) { cg_d[k] = dsum; cg_b[k] = bits; }          // the TU's cbf bit waits for the group decision
            else if (any) ex.atomic_or(&s.cbf[l.plane], 1u << l.tile0);
        }
    });
    if (cg_lam_q4 > 0) ex.phase([&](int tid) {      // coefficient groups: keep or drop
        const int nbl = 1 << (2 * rg.log2n - 3), per_l = 1 << (rg.log2n - 2), per_c = per_l >> 1;
        for (int k = tid; k < nblk; k += NT) {
            const int idx = rg.block_index(k);
            SampleLoc l = unpack_loc(s.desc[idx], idx);
            if (!l.log2n || l.intra || !cg_b[k]) continue;
            const int mate = k ^ (k < nbl ? per_l : per_c);          // the block above / below in the same 4x4 group
            const long long d = cg_d[k] + cg_d[mate];
            const int bits = cg_b[k] + cg_b[mate] + R_SB, tsh = 2 * (15 - bit_depth - l.log2n);
            if (16 * d < ((((long long)cg_lam_q4 * bits) >> 4) << tsh)) {
                store_rows(s.lvl, l, kZero);
                store_pairs(l, kZero);
            } else ex.atomic_or(&s.cbf[l.plane], 1u << l.tile0);
        }
    });
    if (sign_hide) ex.phase([&](int tid) {      // sign data hiding: the forward coefficients are still in `coef`, the scaled levels in `tmp`
        for (int k = tid; k < nblk; k += NT) {
            const int idx = rg.block_index(k);
            SampleLoc l = unpack_loc(s.desc[idx], idx);
            if (!l.log2n || (l.y & 3)) continue;
            int lv[16], c[16];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                uint32_t l2[2], c2[2];
                load_x2(s.lvl + l.base + (l.y + j) * l.stride + l.x, l2);
                load_x2(s.coef + l.base + (l.y + j) * l.stride + l.x, c2);
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    lv[j * 4 + i] = (int)(int16_t)(l2[i >> 1] >> (16 * (i & 1)));
                    c[j * 4 + i] = (int)(int16_t)(c2[i >> 1] >> (16 * (i & 1)));
                }
            }
            const Quantiser qz(l.plane ? qp_c : qp, bit_depth, l.log2n, l.intra, s.quant_scale, s.level_scale);
            int nv = 0;
            const int p = sdh_adjust_scan(l.scan, lv, c, qz, nv);
            if (p < 0) continue;
            const int y = l.y + (p >> 2), x = l.x + (p & 3);
            s.lvl[l.base + y * l.stride + x] = (int16_t)nv;
            s.tmp[l.base + (y & ~1) * l.stride + 2 * x + (y & 1)] = (int16_t)qz.dequant(nv);
        }
    });
    ex.phase([&](int tid) {      // inverse stage 1: columns, shift 7, clip to 16 bit (8.6.4.2)
        for (int k = tid; k < nblk; k += NT) {
            const int idx = rg.block_index(k);
            SampleLoc l = unpack_loc(s.desc[idx], idx);
            if (!l.log2n || !((s.cbf[l.plane] >> l.tile0) & 1)) continue;     // a TU without levels reconstructs to zero: nothing to invert
            int acc[2][4] = {};
            col_stage(s.mq, l, acc);
            round8(acc, [](int v) { return clip3(-32768, 32767, (v + 64) >> 7); });
            store_rows(s.coef, l, acc);
        }
    });
    ex.phase([&](int tid) {      // inverse stage 2: rows, shift 20 - bitDepth
        for (int k = tid; k < nblk; k += NT) {
            const int idx = rg.block_index(k);
            SampleLoc l = unpack_loc(s.desc[idx], idx);
            int acc[2][4] = {};
            if (!l.log2n || !((s.cbf[l.plane] >> l.tile0) & 1)) { store_rows(s.res, l, kZero); continue; }
            const int sh = 20 - bit_depth;
            row_stage(s.mq, s.coef, l, acc);
            round8(acc, [&](int v) { return (int)(int16_t)((v + (1 << (sh - 1))) >> sh); });
            store_rows(s.res, l, acc);
        }
    });
}

// the pair tables, built at compile time: every CTU program used to rebuild them from the byte matrix with a runtime division per entry
// (~400 VALU instructions per lane of every workgroup: 7 % of k_inter_ctu's instruction count, profiles/r02_a phase table)
struct PairTables { uint32_t mp[680], mq[680]; };
constexpr PairTables make_pair_tables()
{
    PairTables t{};
    const Tables m = make_tables();
    for (int i = 0; i < 680; i++) {
        const int lg = i < 8 ? 2 : i < 40 ? 3 : i < 168 ? 4 : 5, n = 1 << lg, off = lg == 2 ? 0 : lg == 3 ? 8 : lg == 4 ? 40 : 168, k = i - off, p = k / n, c = k % n, st = 5 - lg;
        t.mp[i] = (uint32_t)(uint16_t)(int16_t)m.mat[c << st][2 * p] | (uint32_t)(uint16_t)(int16_t)m.mat[c << st][2 * p + 1] << 16;
        t.mq[i] = (uint32_t)(uint16_t)(int16_t)m.mat[(2 * p) << st][c] | (uint32_t)(uint16_t)(int16_t)m.mat[(2 * p + 1) << st][c] << 16;
    }
    return t;
}
DEVCONST PairTables g_pair = make_pair_tables();

// one lane's share of the set-up, for a caller that folds it into a phase of its own (nothing else may touch the fields in that phase)
DEV void residual_init_lane(ResidualShared &s, int tid)
{
    for (int i = tid; i < 680; i += NT) { s.mp[i] = g_pair.mp[i]; s.mq[i] = g_pair.mq[i]; }
    if (tid < 16) { s.tu_log2[tid] = 0; s.tu_intra[tid] = 0; }
    if (tid < 6) { s.quant_scale[tid] = g_tab.quant_scale[tid]; s.level_scale[tid] = g_tab.level_scale[tid]; }
    if (tid < 3) s.cbf[tid] = 0;
}
template <class Ex> DEV void residual_init(Ex &ex, ResidualShared &s)
{
    ex.phase([&](int tid) { residual_init_lane(s, tid); });
}

// K3 for 4x4 TUs alone (k_transform4_blocks, the mihevc_k_transform_sdh entry for log2n 2): NT / 16 blocks from `first` on, 16 lanes per block,
// matrix M (DST-VII when dst, else DCT), every block's group in scan `scan` with sign data hiding when sign_hide
struct Transform4Shared {
    int16_t M[16];
    Block4 blk[NT / 16];
};
template <class Ex>
DEV void transform4_program(Ex &ex, Transform4Shared &s, const int16_t *res, int16_t *lvl, int16_t *rec, int n_blocks, int first, int qp, int bit_depth,
                            int intra, int dst, int scan, int sign_hide)
{
    const Quantiser qz(qp, bit_depth, 2, intra, g_tab.quant_scale, g_tab.level_scale);
    ex.phase([&](int tid) {
        const int g = tid >> 4, i = tid & 15, blk = first + g;
        if (tid < 16) s.M[tid] = dst ? g_tab.dst4[tid >> 2][tid & 3] : g_tab.mat[(tid >> 2) * 8][tid & 3];
        if (i == 0) s.blk[g].nz = 0;
        s.blk[g].res[i] = blk < n_blocks ? res[(size_t)blk * 16 + i] : (int16_t)0;
    });
    ex.phase([&](int tid) { core4_fwd_rows(s.M, s.blk[tid >> 4], tid & 15, bit_depth); });
    ex.phase([&](int tid) { core4_fwd_cols_quant(ex, s.M, s.blk[tid >> 4], tid & 15, qz, sign_hide != 0); });
    if (sign_hide) ex.phase([&](int tid) { if (!(tid & 15)) core4_sign_hide(s.blk[tid >> 4], scan, qz); });
    ex.phase([&](int tid) { core4_inv_cols(s.M, s.blk[tid >> 4], tid & 15, qz); });
    ex.phase([&](int tid) {
        const int g = tid >> 4, i = tid & 15, blk = first + g;
        const int r = core4_inv_rows(s.M, s.blk[g], i, bit_depth);
        if (blk >= n_blocks) return;
        lvl[(size_t)blk * 16 + i] = s.blk[g].lvl[i];
        rec[(size_t)blk * 16 + i] = (int16_t)r;
    });
}

// coefficient-rate estimate of one 4x4 sub-block of levels, in 1/16 bit (oracle/hevc_oracle.c code_tu)
DEV int subblock_bits_q4(const int16_t *lv, int stride)
{
    int bits = 0, any = 0;
    for (int y = 0; y < 4; y++)
        for (int x = 0; x < 4; x++) {
            int a = iabs(lv[y * stride + x]);
            if (!a) continue;
            any = 1;
            bits += rate_level(a);
        }
    return any ? bits + R_SB : 0;
}

}  // namespace mihevc
