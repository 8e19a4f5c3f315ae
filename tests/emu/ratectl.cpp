// tests/emu/ratectl.cpp — TEST HARNESS, NOT PRODUCT (part of tests/emu/libkernel_emu.so).  The rate controller of hevc_amd/csrc/ratectl.h (mihevc::RateControl and
// the GOP structure functions) on plain arrays, call for call as a session makes them (tests/test_ratectl_cpu.py).  No logic here: every entry unpacks its
// arrays, makes the one call and packs the answer.  hevc_amd/ never loads this library.
#include "../../hevc_amd/csrc/ratectl.h"

namespace {

// n frame records from flat arrays (FrameRec's slice-local fields are the session's, not the controller's: left at their defaults)
std::vector<mihevc::FrameRec> records(int n, const int *qp, const int *type, const long long *bits, const unsigned long long *est, const int *est_known)
{
    std::vector<mihevc::FrameRec> v((size_t)std::max(0, n));
    for (int j = 0; j < n; j++) { v[(size_t)j].qp = qp[j]; v[(size_t)j].type = type[j]; v[(size_t)j].bits = bits[j]; v[(size_t)j].est_q4 = est[j]; v[(size_t)j].est_known = est_known[j] != 0; }
    return v;
}

}  // namespace

extern "C" {

// cfg fields the controller reads: qp (>= 0: constant QP, rate control off), vbv_maxrate_kbps, vbv_bufsize_kbits, fps_num / fps_den, b_qp_offset
void *emu_rc_create(int cfg_qp, int maxrate_kbps, int bufsize_kbits, int fps_num, int fps_den, int b_qp_offset, int qp_i, int qp_p, double share, int p_slots)
{
    mihevc_config cfg{};
    cfg.qp = cfg_qp; cfg.vbv_maxrate_kbps = maxrate_kbps; cfg.vbv_bufsize_kbits = bufsize_kbits; cfg.fps_num = fps_num; cfg.fps_den = fps_den; cfg.b_qp_offset = b_qp_offset;
    auto *rc = new mihevc::RateControl();
    rc->init(cfg, qp_i, qp_p, share, p_slots);
    return rc;
}
void emu_rc_destroy(void *h) { delete (mihevc::RateControl *)h; }

void emu_rc_begin_chunk(void *h, int bf, const int *glen, int gops) { ((mihevc::RateControl *)h)->begin_chunk(bf != 0, std::vector<int>(glen, glen + gops)); }

// n: records of steps [0, n) (the session passes t of them at a P step under rate control, none otherwise)
int emu_rc_step_qp(void *h, int g, int t, int n, const int *qp, const int *type, const long long *bits, const unsigned long long *est, const int *est_known)
{
    return ((mihevc::RateControl *)h)->step_qp(g, t, records(n, qp, type, bits, est, est_known));
}

int emu_rc_want_idr(void *h, int g, unsigned long long est, int qa) { return ((mihevc::RateControl *)h)->want_idr(g, est, qa); }
int emu_rc_trial_qp(int want) { return mihevc::RateControl::trial_qp(want); }
int emu_rc_redo_idr(int want, int qa) { return mihevc::RateControl::redo_idr(want, qa) ? 1 : 0; }
void emu_rc_measure_rho(void *h, int n, const unsigned long long *est_p, const int *qp_trial, const unsigned long long *est_i, const int *qa)
{
    ((mihevc::RateControl *)h)->measure_rho(std::vector<unsigned long long>(est_p, est_p + n), std::vector<int>(qp_trial, qp_trial + n),
                                            std::vector<unsigned long long>(est_i, est_i + n), std::vector<int>(qa, qa + n));
}
void emu_rc_idr_settled(void *h, const int *qp, int n) { ((mihevc::RateControl *)h)->idr_settled(std::vector<int>(qp, qp + n)); }

// lane g's records are entries [off[g], off[g + 1]) of the flat arrays
void emu_rc_learn(void *h, int lanes, const int *off, const int *qp, const int *type, const long long *bits, const unsigned long long *est, const int *est_known)
{
    std::vector<std::vector<mihevc::FrameRec>> v((size_t)lanes);
    for (int g = 0; g < lanes; g++) v[(size_t)g] = records(off[g + 1] - off[g], qp + off[g], type + off[g], bits + off[g], est + off[g], est_known + off[g]);
    ((mihevc::RateControl *)h)->learn(v);
}

// the learned state: d = ratio_i, ratio_p, rho_pi, beta_bp; i = idr_qp_hint, rho_measured, rc_on, kQpB (the setter leaves rc_on and kQpB alone: init decides them)
void emu_rc_get_state(void *h, double *d, int *i)
{
    const auto *rc = (const mihevc::RateControl *)h;
    d[0] = rc->ratio_i; d[1] = rc->ratio_p; d[2] = rc->rho_pi; d[3] = rc->beta_bp;
    i[0] = rc->idr_qp_hint; i[1] = rc->rho_measured ? 1 : 0; i[2] = rc->rc_on ? 1 : 0; i[3] = rc->kQpB;
}
void emu_rc_set_state(void *h, const double *d, const int *i)
{
    auto *rc = (mihevc::RateControl *)h;
    rc->ratio_i = d[0]; rc->ratio_p = d[1]; rc->rho_pi = d[2]; rc->beta_bp = d[3];
    rc->idr_qp_hint = i[0]; rc->rho_measured = i[1] != 0;
}

// out: pos, type, cur, prev, nxt, ref_pos
void emu_rc_gop_step(int bf, int t, int len, int *out)
{
    const mihevc::GopStep s = mihevc::gop_step(bf != 0, t, len);
    out[0] = s.pos; out[1] = s.type; out[2] = s.cur; out[3] = s.prev; out[4] = s.nxt; out[5] = s.ref_pos;
}

}  // extern "C"
