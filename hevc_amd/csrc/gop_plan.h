// hevc_amd/csrc/gop_plan.h — GOP layout of one chunk: host policy, pure arithmetic (no HIP; tests/emu/gop_plan.cpp runs it on arrays).
//
// Scene cuts (x265 scenecut + min-keyint, reference core/transcoder.py:401) divide the chunk into segments; every segment is coded as the FEWEST
// closed GOPs keyint allows (the IDR count of an IDR-every-keyint layout), of near-equal length when gop_balance is set: the lanes of the
// lock-step pipeline then run out together instead of idling behind a short last GOP (a 300-picture clip at keyint 90 is 4 x 75 steps, not
// 90 steps of which 60 drive three lanes).  With gop_balance 0 a segment's IDRs sit every keyint pictures.
// The cut detector is the mean absolute difference of every 4th sample of every 4th row between consecutive source pictures (k_scene_diff, one
// launch for the chunk): a cut is a difference above kCutAbs grey levels that is also kCutRatio times the running mean over the ordinary
// pictures before it, taken when every GOP of the segment it closes keeps at least min-keyint pictures.
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

namespace mihevc {

constexpr double kCutAbs = 8.0;          // scene cut: mean absolute difference of consecutive pictures above this many grey levels (8-bit scale) ...
constexpr double kCutRatio = 1.8;        // ... and this many times the running mean over the ordinary pictures before it

// lanes by GOP length, longest first: the lanes that still have a picture at step t are then a prefix [0, batch[t])
struct GopLayout {
    std::vector<int> gstart, glen, prev_len;      // per lane: first picture (place in the chunk), length, length of the GOP before it in the stream
    std::vector<int> batch;                       // per step: lanes with a picture
};

// what the planner carries from chunk to chunk
struct GopState {
    double scene_avg = 0;                     // running mean of the picture-to-picture difference over ordinary pictures (scene-cut detector)
    int last_gop_len = 0;                     // length of the stream's previous GOP (picture timing SEI at the next IDR)
};

// diff: the difference sums of the chunk's n pictures (diff[i] for the pair (i - 1, i), diff[0] unused), EMPTY when cut detection is off; per: what
// turns a sum into a mean on the 8-bit scale; flushing: the stream's last chunk (its last GOP may end short of min_keyint)
inline GopLayout gop_plan(const std::vector<unsigned long long> &diff, double per, int n, int keyint, int min_keyint, bool gop_balance, bool flushing, int max_lanes,
                          GopState &st)
{
    auto gops_of = [keyint](int len) { return (len + keyint - 1) / keyint; };
    std::vector<int> seg{0};                  // segment starts
    if (!diff.empty()) {
        int total = 0;                        // GOPs of the closed segments
        // Until the running mean has seen an ordinary picture (a session's first pictures) the chunk's MEDIAN difference stands in for it: a cut or a
        // flash at the session's second picture is then a jump like any other and never becomes the mean the next pictures are measured against
        double median = 0;
        if (st.scene_avg <= 0) {
            std::vector<unsigned long long> sorted(diff.begin() + 1, diff.end());
            std::nth_element(sorted.begin(), sorted.begin() + (ptrdiff_t)(sorted.size() / 2), sorted.end());
            median = (double)sorted[sorted.size() / 2] / per;
        }
        auto is_jump = [&](int i) {
            const double d = (double)diff[(size_t)i] / per, base = st.scene_avg > 0 ? st.scene_avg : median;
            return d > kCutAbs && d > kCutRatio * base;
        };
        for (int i = 1; i < n; i++) {
            const double d = (double)diff[(size_t)i] / per;
            const int len = i - seg.back(), g = gops_of(len);
            const bool jump = is_jump(i);
            // a run of jumps (a flash: into the odd picture and out of it again) is cut at its LAST picture: the GOP then starts on the scene that stays,
            // not on the flash it would have to predict everything from
            const bool last_of_run = !(i + 1 < n && is_jump(i + 1));
            const int shortest = gop_balance ? len / g : (len % keyint ? len % keyint : keyint);
            // the GOP the cut opens must keep min-keyint pictures too: the next chunk starts with an IDR picture of its own (the stream's last chunk may end short)
            const bool tail_ok = flushing || n - i >= std::max(1, min_keyint);
            if (jump && last_of_run && tail_ok && shortest >= std::max(1, min_keyint) && total + g + gops_of(n - i) <= max_lanes) { total += g; seg.push_back(i); }
            if (!jump) st.scene_avg = st.scene_avg > 0 ? 0.8 * st.scene_avg + 0.2 * d : d;      // ordinary pictures only: a jump says nothing about the new scene's motion
        }
    }
    std::vector<int> gstart_stream;
    for (size_t k = 0; k < seg.size(); k++) {
        const int a0 = seg[k], len = (k + 1 < seg.size() ? seg[k + 1] : n) - a0, g = gops_of(len);
        if (gop_balance)
            for (int j = 0, at = a0; j < g; at += len / g + (j < len % g), j++) gstart_stream.push_back(at);
        else
            for (int at = a0; at < a0 + len; at += keyint) gstart_stream.push_back(at);
    }
    const int gops = (int)gstart_stream.size();
    GopLayout gl;
    std::vector<int> order((size_t)gops);
    gl.gstart.assign((size_t)gops, 0); gl.glen.assign((size_t)gops, 0); gl.prev_len.assign((size_t)gops, 0);
    for (int g = 0; g < gops; g++) order[(size_t)g] = g;
    auto len_of = [&](int k) { return (k + 1 < gops ? gstart_stream[(size_t)k + 1] : n) - gstart_stream[(size_t)k]; };
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return len_of(a) > len_of(b); });
    for (int g = 0; g < gops; g++) {
        const int k = order[(size_t)g];
        gl.gstart[(size_t)g] = gstart_stream[(size_t)k]; gl.glen[(size_t)g] = len_of(k);
        gl.prev_len[(size_t)g] = k > 0 ? len_of(k - 1) : st.last_gop_len;
    }
    st.last_gop_len = len_of(gops - 1);
    gl.batch.assign((size_t)gl.glen[0], 0);
    for (int g = 0; g < gops; g++)
        for (int t = 0; t < gl.glen[(size_t)g]; t++) gl.batch[(size_t)t] = g + 1;
    return gl;
}

}  // namespace mihevc
