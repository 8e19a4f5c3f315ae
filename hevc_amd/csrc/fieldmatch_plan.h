// hevc_amd/csrc/fieldmatch_plan.h — the decisions of inverse telecine (mihevc_send_frame_fieldmatch): host policy, pure arithmetic over the
// metrics of k_fm_metrics (no HIP; tests/emu/fieldmatch.cpp runs it on arrays).
//   match      the candidate m in {c, p, n} with the least comb sum S_m; ties resolve in the order c, p, n
//   fallback   K_match > kFmCombBlock and the caller set `deint`: the frame's picture is the deinterlacer's, not the weave
//   decimate   frames are taken in cycles of kFmCycle counted from the clip's first frame; the frame of a cycle with the least (DB, DS), compared
//              lexicographically with ties to the lowest index, is dropped; a last cycle with fewer frames drops nothing.  The clip's first frame carries
//              all-ones in both (fm_first_frame): it is never the duplicate
#pragma once
#include <cstdint>

namespace mihevc {

constexpr uint32_t kFmCombBlock = 80;     // combed samples in one 16 x 16 block above which a match counts as combed
constexpr int kFmCycle = 5;               // 3:2 pulldown: five frames carry four film frames

struct FmMetrics {
    uint64_t comb_sum[3];                 // S_c, S_p, S_n
    uint32_t comb_block[3];               // K_c, K_p, K_n
    uint64_t dup_sum;                     // DS
    uint32_t dup_block;                   // DB
};

// from the eight numbers of k_fm_fold (S_c S_p S_n K_c K_p K_n DS DB)
inline FmMetrics fm_metrics_of(const unsigned long long *v)
{
    FmMetrics m;
    for (int i = 0; i < 3; i++) { m.comb_sum[i] = v[i]; m.comb_block[i] = (uint32_t)v[3 + i]; }
    m.dup_sum = v[6]; m.dup_block = (uint32_t)v[7];
    return m;
}
inline void fm_first_frame(FmMetrics &m) { m.dup_sum = ~(uint64_t)0; m.dup_block = ~(uint32_t)0; }

inline int fm_match(const FmMetrics &m)
{
    int best = 0;
    for (int i = 1; i < 3; i++)
        if (m.comb_sum[i] < m.comb_sum[best]) best = i;
    return best;
}
inline bool fm_falls_back(const FmMetrics &m, int match, bool deint) { return deint && m.comb_block[match] > kFmCombBlock; }

// the frame of a complete cycle that is dropped: index into cycle[0 .. kFmCycle - 1]
inline int fm_drop(const FmMetrics *cycle)
{
    int best = 0;
    for (int i = 1; i < kFmCycle; i++)
        if (cycle[i].dup_block < cycle[best].dup_block || (cycle[i].dup_block == cycle[best].dup_block && cycle[i].dup_sum < cycle[best].dup_sum)) best = i;
    return best;
}

}  // namespace mihevc
