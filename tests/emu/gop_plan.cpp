// tests/emu/gop_plan.cpp — TEST HARNESS, NOT PRODUCT (part of tests/emu/libkernel_emu.so).  The GOP planner of hevc_amd/csrc/gop_plan.h on plain arrays, as a
// session calls it once per chunk (tests/test_gop_plan_cpu.py; under ASAN + UBSAN in tests/sanitize_cpu.sh).  hevc_amd/ never loads this library.
#include "../../hevc_amd/csrc/gop_plan.h"

extern "C" {

// diff: n_diff difference sums (0: cut detection off, else n).  scene_avg, last_gop_len: the planner's state, read and written.  gstart, glen, prev_len: room
// for n lanes; batch: room for n steps.  Returns the number of lanes; *steps = entries of batch.
int emu_gop_plan(const unsigned long long *diff, int n_diff, double per, int n, int keyint, int min_keyint, int gop_balance, int flushing, int max_lanes,
                 double *scene_avg, int *last_gop_len, int *gstart, int *glen, int *prev_len, int *batch, int *steps)
{
    if (n < 1 || keyint < 1 || (n_diff != 0 && n_diff != n)) return -3;
    mihevc::GopState st;
    st.scene_avg = *scene_avg; st.last_gop_len = *last_gop_len;
    const mihevc::GopLayout gl = mihevc::gop_plan(std::vector<unsigned long long>(diff, diff + n_diff), per, n, keyint, min_keyint, gop_balance != 0, flushing != 0, max_lanes, st);
    *scene_avg = st.scene_avg; *last_gop_len = st.last_gop_len;
    const int gops = (int)gl.glen.size();
    for (int g = 0; g < gops; g++) { gstart[g] = gl.gstart[(size_t)g]; glen[g] = gl.glen[(size_t)g]; prev_len[g] = gl.prev_len[(size_t)g]; }
    *steps = (int)gl.batch.size();
    for (int t = 0; t < *steps; t++) batch[t] = gl.batch[(size_t)t];
    return gops;
}

}  // extern "C"
