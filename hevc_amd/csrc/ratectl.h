// hevc_amd/csrc/ratectl.h — rate-control policy of a session (VBV-capped constant quality, one controller per GOP lane: DESIGN.md §5b), and the GOP structure
// it plans over.  Host-only and lock-free: the session does the device work (analyses, trial, redo launches, estimates summed over the slices of a picture) and
// hands in numbers and copies of the frame records; this unit decides QPs and learns from finished chunks.  Every input is deterministic.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "../../include/mihevc.h"

namespace mihevc {

constexpr int kIdrStart = 5;  // first chunk of a session: IDR pictures under rate control are analysed at the CRF's IDR QP + 5, then re-analysed only
                              // where the rate model asks for a QP at least kIdrRedo away (round 1 analysed every IDR at three QPs: 23 % of device time)
constexpr int kIdrRedo = 2;
constexpr double kBudgetShare = 0.985;   // a GOP is planned to 98.5 % of vbv-maxrate x its duration: the estimate-to-CABAC ratio is known to ~1 %
constexpr double kCpbStart = 0.9;        // CPB fullness every closed GOP may assume at its IDR (= the buffering period SEI's initial delay)
constexpr double kIdrCpbShare = 0.85;    // an IDR picture may take at most this share of that fullness

// cfg.bframes: a closed GOP of `len` pictures is coded I0 P2 b1 P4 b3 ...: step 0 the IDR picture, odd steps the anchors (P), even steps the B picture between the
// last two anchors; the GOP's last picture is always an anchor.  Without B pictures step = display position.  Step t codes the picture at display position `pos`,
// slice type `type` (2 I, 1 P, 0 B), into reconstruction buffer `cur`: anchor number k (the IDR picture is 0) into k & 1, predicting from the other one (`prev`);
// a B picture into 2, predicting from the anchors either side (`prev`, `nxt`).  ref_pos: display position of the list-0 reference (not read at the IDR picture).
struct GopStep { int pos, type, cur, prev, nxt, ref_pos; };
inline int pos_of_step(bool bf, int t, int len) { return !bf || t == 0 ? t : (t & 1) ? std::min(t + 1, len - 1) : t - 1; }
inline int type_of_step(bool bf, int t) { return t == 0 ? 2 : (bf && !(t & 1)) ? 0 : 1; }
inline GopStep gop_step(bool bf, int t, int len)
{
    const int pos = pos_of_step(bf, t, len), type = type_of_step(bf, t), anchor = !bf ? t : (t + 1) / 2;
    if (type == 0) return GopStep{pos, type, 2, (t / 2 - 1) & 1, (t / 2) & 1, pos - 1};
    return GopStep{pos, type, anchor & 1, (anchor & 1) ^ 1, 0, !bf ? pos - 1 : pos_of_step(bf, std::max(0, t - 2), len) * (t > 1)};
}

// what the session knows about one coded picture.  With slices that share one rate plan (group): bits / est_q4 are sums over the slices, bits_local this slice's
struct FrameRec { int qp = 0, type = 0; long long bits = -1, bits_local = -1; unsigned long long est_q4 = 0, est_local = 0; bool est_known = false; };

class RateControl {
public:
    // learned over the session (updated once per chunk: deterministic)
    bool rc_on = false;
    double ratio_i = 1.0, ratio_p = 1.0;      // (CABAC bits) / (device estimate)
    bool rho_measured = false;                // the session's first chunk measures rho with a trial analysis of the GOPs' first P picture
    double rho_pi = 1.0 / 16.0;               // (P bits) / (IDR bits) at equal QP: the prior before a GOP's first P estimate lands
    double beta_bp = 0.45;                    // cfg.bframes: (B bits at QP + kQpB) / (P bits at QP): what a B picture takes of the GOP budget beside a P picture
    int idr_qp_hint = -1;                     // mean IDR QP the last chunk settled on: where the next chunk's IDR analysis starts
    int kQpB = 2;                             // a B picture takes the QP of the anchors around it + kQpB (x265 pbratio 1.3): nothing predicts from it

    // share: the part of the picture's rate and buffer this session plans with (one slice of several); p_slots: a P step's CABAC size is known p_slots steps later
    void init(const mihevc_config &cfg, int qp_i, int qp_p, double share, int p_slots)
    {
        cfg_ = cfg; qp_i_ = qp_i; qp_p_ = qp_p; share_ = share; p_slots_ = p_slots;
        rc_on = cfg.qp < 0 && cfg.vbv_maxrate_kbps > 0;
        kQpB = cfg.b_qp_offset >= 0 ? std::min(8, cfg.b_qp_offset) : 2;
    }

    // CPB model (x265 nal-hrd=vbr + vbv-maxrate / vbv-bufsize, reference core/transcoder.py:399-400).  The GOPs of a chunk are coded in
    // lock-step, so a GOP cannot know the buffer level its predecessor leaves.  Every closed GOP is therefore planned to be buffer-neutral:
    // it may assume the fullness kCpbStart x bufsize at its IDR (what the buffering period SEI announces for the first one), its IDR takes at
    // most kIdrCpbShare of that, and its pictures together take at most kBudgetShare of what the channel delivers during the GOP — so the
    // level at the next IDR is at least the assumed one again (tests replay the produced sizes through the Annex C arrival / removal schedule).
    void begin_chunk(bool bf, const std::vector<int> &glen)
    {
        const double fps = (double)cfg_.fps_num / cfg_.fps_den;
        bf_ = bf;
        gop_len_ = glen;
        qp_prev_.assign(glen.size(), qp_p_);
        budget_.assign(glen.size(), 0.0);
        for (size_t g = 0; g < glen.size(); g++) budget_[g] = kBudgetShare * share_ * cfg_.vbv_maxrate_kbps * 1000.0 * gop_len_[g] / fps;
        cpb_idr_cap_ = cfg_.vbv_bufsize_kbits > 0 ? kIdrCpbShare * kCpbStart * share_ * cfg_.vbv_bufsize_kbits * 1000.0 : 1e30;
    }

    // QP of lane g's picture at step t.  IDR pictures: the first analysis (under rate control where the last chunk's IDR pictures ended; first chunk: kIdrStart
    // above the CRF's IDR QP).  A B picture: the QP of the last anchor + kQpB; it does not move the controller's walk.  gop[j]: the lane's record of step j < t
    // (read for P pictures under rate control only)
    int step_qp(int g, int t, const std::vector<FrameRec> &gop)
    {
        const int type = type_of_step(bf_, t);
        const int qp = t == 0 ? (!rc_on ? qp_i_ : std::min(51, std::max(qp_i_, idr_qp_hint >= 0 ? idr_qp_hint : qp_i_ + kIdrStart)))
                              : type == 0 ? std::min(51, qp_prev_[g] + kQpB) : (rc_on ? decide_p(g, t, gop) : qp_p_);
        if (type != 0) qp_prev_[g] = qp;
        return qp;
    }

    // ONE analysis per IDR picture, then the rate model decides: IDR bits scale as 2^(-dQP/6) around the analysed point, P size at the IDR's QP is rho x IDR
    // size, the rest of the GOP budget is shared by the P pictures; wanted is the IDR QP whose predicted steady P QP sits 3 above it (the usual I/P offset),
    // never finer than the CRF asks, and whose picture fits the share of the CPB an IDR may take.  est: lane g's IDR estimate (q4 bits) analysed at QP qa.
    int want_idr(int g, unsigned long long est, int qa) const
    {
        const double ib_a = std::max(1.0, (double)est / 16.0 * ratio_i);
        int pick = 51;
        double best_d = 1e30;
        for (int q = qp_i_; q <= 51; q++) {
            const double ib = ib_a * std::exp2((qa - q) / 6.0), rest = budget_[g] - ib;
            double d;
            if (ib > cpb_idr_cap_ && q < 51) continue;
            if (gop_len_[g] < 2) d = ib <= budget_[g] ? -1e9 + q : 1e9 + ib;          // IDR-only GOP: finest that fits
            else if (rest <= 0) d = 1e9 + ib;
            else {
                double units = 0;              // the GOP's other pictures in units of a P picture (cfg.bframes: a B picture counts beta_bp)
                for (int j = 1; j < gop_len_[g]; j++) units += type_of_step(bf_, j) == 1 ? 1.0 : beta_bp;
                const double q_ss = std::max((double)qp_p_, q + 6.0 * std::log2(ib * rho_pi / (rest / std::max(0.5, units))));
                d = std::fabs(q_ss - (q + 3));
            }
            if (d < best_d) { best_d = d; pick = q; }
        }
        return pick;
    }
    // the rho trial (first chunk of a session): every GOP's first P picture analysed at the wanted IDR QP + 3 against the unfiltered IDR analysis
    static int trial_qp(int want) { return std::min(51, want + 3); }
    // both estimates brought to one QP: the P picture (est_p) from its trial QP, the IDR picture (est_i) from the QP it was analysed at
    void measure_rho(const std::vector<unsigned long long> &est_p, const std::vector<int> &qp_trial, const std::vector<unsigned long long> &est_i, const std::vector<int> &qa)
    {
        double lg = 0;
        int nl = 0;
        for (size_t g = 0; g < est_p.size(); g++) {
            const unsigned long long ep = est_p[g];
            if (!ep || !est_i[g]) continue;
            lg += std::log2((double)ep / (double)est_i[g]) + (qp_trial[g] - qa[g]) / 6.0;
            nl++;
        }
        if (nl) rho_pi = std::min(1.0, std::max(1.0 / 256, std::exp2(lg / nl)));
        rho_measured = true;
    }
    // lanes whose wanted QP is kIdrRedo or more away from the analysed one are analysed again, at that QP
    static bool redo_idr(int want, int qa) { return std::abs(want - qa) >= kIdrRedo; }
    // the IDR QPs lanes [0, qp.size()) settled on
    void idr_settled(const std::vector<int> &qp)
    {
        int sum_q = 0, B = (int)qp.size();
        for (int g = 0; g < B; g++) { qp_prev_[g] = qp[g]; sum_q += qp[g]; }
        idr_qp_hint = (sum_q + B / 2) / B;
    }

    // learn from the finished chunk (all CABAC sizes are known now, so this is deterministic): CABAC bits per estimated bit for I and P pictures, the P/I size
    // ratio at equal QP, and what a B picture takes beside a P picture.  lanes[g][j]: lane g's record of step j
    void learn(const std::vector<std::vector<FrameRec>> &lanes)
    {
        double bi = 0, ei = 0, bp = 0, ep = 0, lg = 0, lgb = 0;
        int np = 0, nb = 0;
        for (size_t g = 0; g < lanes.size(); g++) {
            const auto &idr = lanes[g][0];
            if (idr.bits < 0 || !idr.est_q4) continue;
            bi += (double)idr.bits; ei += (double)idr.est_q4 / 16.0;
            for (int j = 1; j < gop_len_[g]; j++) {          // steps: decoding order
                const auto &fr = lanes[g][(size_t)j];
                if (fr.bits <= 0 || !fr.est_q4) continue;
                bp += (double)fr.bits; ep += (double)fr.est_q4 / 16.0;
                if (type_of_step(bf_, j) == 1) { lg += std::log2((double)fr.bits / (double)idr.bits) + (fr.qp - idr.qp) / 6.0; np++; }
                else { lgb += std::log2((double)fr.bits / (double)idr.bits) + (fr.qp - kQpB - idr.qp) / 6.0; nb++; }
            }
        }
        if (ei > 0) ratio_i = 0.5 * ratio_i + 0.5 * bi / ei;
        if (ep > 0) ratio_p = 0.5 * ratio_p + 0.5 * bp / ep;
        if (np) rho_pi = std::min(1.0, std::max(1.0 / 256, 0.5 * rho_pi + 0.5 * std::exp2(lg / np)));
        // a B picture at QP + kQpB against a P picture at QP (both brought to the IDR picture's QP through the 2^(-dQP/6) rule)
        if (np && nb) beta_bp = std::min(1.5, std::max(0.05, 0.5 * beta_bp + 0.5 * std::exp2(lgb / nb - lg / np)));
    }

private:
    // P-picture QP of lane g at step t.  Every input is deterministic: CABAC sizes only of pictures whose ring slot has been reused (steps <= t - p_slots),
    // device estimates of steps <= t - 2 (the step loop waits for that copy), a model for the picture in flight.  The controller solves for the constant QP
    // that spends the rest of the GOP budget and walks towards it (+3 / -1 per picture, dead band 0.75): a constant QP is what the budget buys the most PSNR with.
    int decide_p(int g, int t, const std::vector<FrameRec> &gop) const
    {
        auto frame = [&](int j) -> const FrameRec & { return gop[(size_t)j]; };
        auto is_p = [&](int j) { return type_of_step(bf_, j) == 1; };
        // CABAC / estimate ratio of this GOP's finished P / B pictures, seeded with two pictures' worth of the session ratio
        double sum_b = 0, sum_e = 0, seed = 0;
        for (int j = 1; j <= t - p_slots_; j++)
            if (frame(j).bits >= 0 && frame(j).est_q4 > 0) { sum_b += (double)frame(j).bits; sum_e += (double)frame(j).est_q4 / 16.0; }
        for (int j = t - 2; j >= 1 && seed == 0; j--) if (frame(j).est_known) seed = 2.0 * (double)frame(j).est_q4 / 16.0;
        const double rp = (sum_e + seed) > 0 ? (sum_b + ratio_p * seed) / (sum_e + seed) : ratio_p;
        // reference point (q_ref, b_ref) of the rate model b(q) = b_ref * 2^((q_ref - q) / 6): the last two P estimates, or the
        // IDR picture scaled by the learned P/I ratio before any P estimate exists.  (cfg.bframes: P pictures only; a B picture is modelled as
        // beta_bp x a P picture at its QP - kQpB.)
        const auto &idr = frame(0);
        const double idr_bits = (double)idr.est_q4 / 16.0 * ratio_i;
        double b_ref = idr_bits * rho_pi, lg = 0;
        int q_ref = idr.qp, have = 0;
        for (int j = t - 2; j >= 1 && have < 2; j--) {
            if (!is_p(j) || !frame(j).est_known) continue;
            const double b = std::max(1.0, (double)frame(j).est_q4 / 16.0 * rp);
            if (!have) q_ref = frame(j).qp;
            lg += std::log2(b) + (frame(j).qp - q_ref) / 6.0;
            have++;
        }
        if (have) b_ref = std::exp2(lg / have);
        double spent = idr_bits;
        for (int j = 1; j < t; j++) {
            const auto &fr = frame(j);
            if (j <= t - p_slots_ && fr.bits >= 0) spent += (double)fr.bits;
            else if (j <= t - 2 && fr.est_known) spent += (double)fr.est_q4 / 16.0 * rp;
            else spent += (is_p(j) ? 1.0 : beta_bp) * b_ref * std::exp2((q_ref - (fr.qp - (is_p(j) ? 0 : kQpB))) / 6.0);
        }
        // what is left of the budget, shared by the pictures still to come in units of a P picture (a B picture counts beta_bp)
        double units = 0;
        for (int j = t; j < gop_len_[g]; j++) units += is_p(j) ? 1.0 : beta_bp;
        double target = (budget_[g] - spent) / std::max(0.5, units);
        target = std::max(target, 0.25 * budget_[g] / gop_len_[g]);
        const double q_ss = q_ref + 6.0 * std::log2(b_ref / target);
        int qp;
        if (t == 1) qp = std::max((int)std::lround(q_ss), idr.qp);    // first P: straight to the model, never finer than its IDR
        else {
            const double d = q_ss - qp_prev_[g];
            qp = qp_prev_[g] + (d >= 0.75 ? std::min(3, (int)std::lround(d)) : d <= -0.75 ? -1 : 0);
        }
        return std::min(std::max(qp, qp_p_), 51);                    // the CRF is the quality ceiling, the VBV only raises QP
    }

    mihevc_config cfg_{};
    int qp_i_ = 0, qp_p_ = 0, p_slots_ = 1;
    double share_ = 1.0;
    // the chunk's lanes
    bool bf_ = false;
    std::vector<int> gop_len_, qp_prev_;
    std::vector<double> budget_;
    double cpb_idr_cap_ = 1e30;
};

}  // namespace mihevc
