// hevc_amd/csrc/stage_args.h — host side of the single-picture stage entries: the kernels' argument blocks built in one place, for the
// mihevc_k_* entries (device.hip) and their stepped twins (tests/emu).  Every builder sets every field of its block; where the planes and
// tables live (device buffers, host vectors) stays with the caller.  The batched blocks of a session (session.cpp) have rules of their own.
// Nothing in kernels/ includes this file.
#pragma once
#include "kernels/common.h"
#include "kernels/inter.h"
#include "kernels/intra.h"
#include "kernels/loopfilter.h"

namespace mihevc {

// the one place that reads the fields of the ABI struct
inline CostParams cost_params_of(const mihevc_cost_params &p, int sign_hide = 0)
{
    return CostParams{p.qp,        p.qp_c,       p.bit_depth,  p.lambda_sad_q4, p.lambda_q4,    p.me_range, p.tile_cols, p.tile_rows, p.intra_nxn,
                      p.intra_in_p, p.pre_search, p.rdo_zero,   p.chroma_modes,  p.mc_top,       p.mc_bottom, p.rdo_cg,   sign_hide};
}

// f(T{}) with T the sample type of the bit depth (uint8_t at 8, uint16_t at 10); MIHEVC_EINVAL for any other depth
template <class F> int with_depth(int bit_depth, F &&f)
{
    if (bit_depth == 8) return f(uint8_t{});
    if (bit_depth == 10) return f(uint16_t{});
    return MIHEVC_EINVAL;
}

inline int ctus_of(int n) { return (n + CTU - 1) / CTU; }

// what an analysis stage writes: CU records ((h/8) x (w/8)), levels (strides w, w/2, w/2), optional rate estimate
struct AnalysisOut {
    mihevc_cu_rec *cu;
    int16_t *coef[3];
    unsigned long long *est;
};

// src, rec, ...: three planes (Y, Cb, Cr).  plan: per CTU, for the two-stage launch of an I picture (nullptr: one workgroup runs both stages)
template <typename T>
IntraArgs<T> intra_args(const Plane<const T> *src, const Plane<T> *rec, int w, int h, const CostParams &prm, const AnalysisOut &out, IntraPlan *plan = nullptr)
{
    IntraArgs<T> a;
    for (int i = 0; i < 3; i++) { a.src[i] = src[i]; a.rec[i] = rec[i]; a.coef[i] = out.coef[i]; }
    a.w = w; a.h = h; a.ctus_w = ctus_of(w); a.ctus_h = ctus_of(h); a.prm = prm;
    a.cu = out.cu; a.diagonal = 0; a.est = out.est; a.sparse_coef = 0; a.ip = nullptr; a.plan = plan;
    return a;
}

// what a stage entry that returns the plan (mihevc_k_intra_plan and its stepped twin) does to the bytes k_intra_plan never writes: mode / cmode of the
// nodes that do not lie wholly inside the picture, and pad, come back as 0
inline void intra_plan_clear_unwritten(mihevc_intra_plan *plan, int w, int h)
{
    for (int cy = 0; cy < ctus_of(h); cy++)
        for (int cx = 0; cx < ctus_of(w); cx++) {
            mihevc_intra_plan &p = plan[cy * ctus_of(w) + cx];
            p.pad = 0;
            for (int nd = 0; nd < 21; nd++) {
                const int q = nd < 5 ? nd - 1 : (nd - 5) >> 2, sub = (nd - 5) & 3, n = nd == 0 ? 32 : nd < 5 ? 16 : 8;      // host form of node_geom
                const int x = nd == 0 ? 0 : (q & 1) * 16 + (nd < 5 ? 0 : (sub & 1) * 8), y = nd == 0 ? 0 : (q >> 1) * 16 + (nd < 5 ? 0 : (sub >> 1) * 8);
                if (cx * CTU + x + n > w || cy * CTU + y + n > h) p.mode[nd] = p.cmode[nd] = 0;
            }
        }
}

// the intra second pass of a P picture on the inter pass's reconstruction, records and levels (tile grid: the P pictures' own, from prm)
template <typename T> IntraArgs<T> intra_in_p_args(const InterArgs<T> &e)
{
    IntraArgs<T> a = intra_args<T>(e.src, e.rec, e.w, e.h, e.prm, AnalysisOut{e.cu, {e.coef[0], e.coef[1], e.coef[2]}, e.est});
    a.ip = e.ip;
    return a;
}

// ref0 / ref1: padded reference planes of list 0 / list 1; ref1 == nullptr: a P picture (no list-1 centres or table).  centers*: per CTU, or nullptr;
// me*: per CTU 21 x (mvx, mvy, cost); ip: per CTU hand-over to the intra second pass, or nullptr
template <typename T>
InterArgs<T> inter_args(const Plane<const T> *src, const Plane<const T> *ref0, const Plane<const T> *ref1, const Plane<T> *rec, int w, int h, const CostParams &prm,
                        const AnalysisOut &out, const int16_t *centers0, const int16_t *centers1, int32_t *me0, int32_t *me1, IpInfo *ip)
{
    InterArgs<T> a;
    for (int i = 0; i < 3; i++) {
        a.src[i] = src[i]; a.ref[i] = ref0[i]; a.rec[i] = rec[i]; a.coef[i] = out.coef[i];
        a.ref1[i] = ref1 ? ref1[i] : Plane<const T>{nullptr, 0};
    }
    a.w = w; a.h = h; a.ctus_w = ctus_of(w); a.prm = prm;
    a.centers = centers0; a.me = me0; a.cu = out.cu; a.est = out.est; a.sparse_coef = 0; a.ip = ip;
    a.centers1 = ref1 ? centers1 : nullptr; a.me1 = ref1 ? me1 : nullptr;
    return a;
}

// search centres of a P picture from the 1/4-size pictures (lsrc, lref: (w/4) x (h/4) each) of its source and reference luma
template <typename T> PreArgs<T> pre_args(const InterArgs<T> &e, uint8_t *lsrc, uint8_t *lref, int16_t *centers)
{
    PreArgs<T> a;
    a.src = e.src[0]; a.ref = e.ref[0]; a.lsrc = lsrc; a.lref = lref; a.w = e.w; a.h = e.h; a.bit_depth = e.prm.bit_depth; a.centers = centers; a.cost = nullptr;
    return a;
}

// dir 0: vertical edges, 1: horizontal edges; y_org: DeblockArgs::y_org (0: a plain picture)
template <typename T> DeblockArgs<T> deblock_args(const Plane<T> *rec, int w, int h, const mihevc_cu_rec *cu, int bit_depth, int dir, int y_org = 0)
{
    DeblockArgs<T> a;
    for (int i = 0; i < 3; i++) a.rec[i] = rec[i];
    a.w = w; a.h = h; a.cu = cu; a.bit_depth = bit_depth; a.dir = dir; a.y_org = y_org;
    return a;
}

// SAO, or with cu the fused loop filter (dbk: the PRE-deblock reconstruction).  halo: bit 0 a slice above, bit 1 below (SaoArgs::halo_top / halo_bottom);
// sse_ctu: SaoArgs::sse_ctu, or nullptr
template <typename T>
SaoArgs<T> sao_args(const Plane<const T> *src, const Plane<const T> *dbk, const Plane<T> *out, int w, int h, const CostParams &prm, mihevc_sao_ctu *sao,
                    const mihevc_cu_rec *cu = nullptr, int halo = 0, uint32_t *sse_ctu = nullptr)
{
    SaoArgs<T> a;
    for (int i = 0; i < 3; i++) { a.src[i] = src[i]; a.dbk[i] = dbk[i]; a.out[i] = out[i]; }
    a.w = w; a.h = h; a.ctus_w = ctus_of(w); a.prm = prm; a.sao = sao; a.sse = nullptr; a.sse_ctu = sse_ctu; a.cu = cu;
    a.halo_top = (halo & 1) ? 1 : 0; a.halo_bottom = (halo & 2) ? 1 : 0;
    return a;
}

// the block of the border pad and of the picture hash kernels, which read only the final planes (padded) and the hash words (`sse`); the rest is zero
template <typename T> SaoArgs<T> picture_args(const Plane<T> *pic, int w, int h, unsigned long long *hash_words = nullptr)
{
    SaoArgs<T> a{};
    for (int i = 0; i < 3; i++) a.out[i] = pic[i];
    a.w = w; a.h = h; a.sse = hash_words;
    return a;
}

}  // namespace mihevc
