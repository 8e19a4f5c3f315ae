// tools/measure_fieldmatch.hip — the numbers DESIGN.md §6h names, device planes in (three frames of pseudo-random samples, as a session's ring holds them): the
// HIP-event time of one k_fm_metrics launch with its fold and of one k_fm_weave launch (5 warm-up launches, then 30 timed ones, each between its own pair of
// events), and the host's wall-clock wait per frame as a session with device-resident sources has it: the three device-to-device copies of the next frame into the
// ring, the metrics, their copy to pinned memory, an event, and the wait for that event.  One JSON line per case with the median, the fastest, the slowest and the
// bytes the metrics read (the luma of C and P once, the other field's rows of N).  A measurement tool, not part of the library; it launches the library's own
// kernels through launch_fm_metrics / launch_fm_weave (csrc/device.h):
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 tools/measure_fieldmatch.hip -Lhevc_amd -lmihevc -Wl,-rpath,'$ORIGIN/../hevc_amd' -o build/measure_fieldmatch
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <vector>

#include "../hevc_amd/csrc/device.h"

using namespace mihevc;

#define CK(x)                                                                              \
    do {                                                                                   \
        hipError_t e_ = (x);                                                               \
        if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } \
    } while (0)

static void stats(std::vector<float> &us, float &med, float &lo, float &hi)
{
    std::sort(us.begin(), us.end());
    med = us[us.size() / 2]; lo = us.front(); hi = us.back();
}

static int run(int w, int h, int depth)
{
    const int pw = (w + 7) & ~7, ph = (h + 7) & ~7;
    const size_t es = depth > 8 ? 2 : 1;
    void *src[4][3], *dst[3];      // three frames of the ring and the caller's next frame
    int ostride[3];
    const int pitch_y = (w + 15) & ~15, pitch_c = (w / 2 + 15) & ~15;
    uint32_t rnd = 2463534242u;
    for (int f = 0; f < 4; f++)
        for (int c = 0; c < 3; c++) {
            const size_t n = (size_t)(c ? pitch_c : pitch_y) * (c ? h / 2 : h);
            std::vector<uint8_t> host(n * es);
            for (size_t i = 0; i < n; i++) {
                rnd = rnd * 1664525u + 1013904223u;
                const unsigned v = (rnd >> 16) & ((1u << depth) - 1);
                if (es == 1) host[i] = (uint8_t)v; else { host[2 * i] = (uint8_t)v; host[2 * i + 1] = (uint8_t)(v >> 8); }
            }
            CK(hipMalloc(&src[f][c], n * es));
            CK(hipMemcpy(src[f][c], host.data(), n * es, hipMemcpyHostToDevice));
        }
    for (int c = 0; c < 3; c++) {
        const int pwo = c ? pw / 2 : pw, pho = c ? ph / 2 : ph;
        ostride[c] = (pwo + 63) & ~63;
        CK(hipMalloc(&dst[c], (size_t)ostride[c] * pho * es));
    }
    const size_t nwg = (size_t)fm_workgroups(w, h);
    unsigned long long *part, *host;
    CK(hipMalloc((void **)&part, (nwg + 1) * 8 * sizeof(unsigned long long)));
    CK(hipHostMalloc((void **)&host, 8 * sizeof(unsigned long long)));
    const FmArgs ma = fm_args(depth, src[0][0], src[1][0], src[2][0], pitch_y, w, h, 0, part);
    const DeintArgs wa = deint_args(depth, src[0], src[1], src[0], pitch_y, pitch_c, w, h, pw, ph, 0, 0, dst, ostride);
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    std::vector<float> m_us, w_us, wait_us;
    for (int i = 0; i < 35; i++) {
        float ms = 0;
        CK(hipEventRecord(e0, 0));
        CK(launch_fm_metrics(0, ma, part + nwg * 8, es == 2));
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        CK(hipEventElapsedTime(&ms, e0, e1));
        if (i >= 5) m_us.push_back(ms * 1000.0f);
        CK(hipEventRecord(e0, 0));
        CK(launch_fm_weave(0, wa, es == 2));
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        CK(hipEventElapsedTime(&ms, e0, e1));
        if (i >= 5) w_us.push_back(ms * 1000.0f);
        const auto t0 = std::chrono::steady_clock::now();
        for (int c = 0; c < 3; c++)
            CK(hipMemcpy2DAsync(src[2][c], (c ? pitch_c : pitch_y) * es, src[3][c], (c ? pitch_c : pitch_y) * es, (size_t)(c ? w / 2 : w) * es, c ? h / 2 : h, hipMemcpyDeviceToDevice, 0));
        CK(launch_fm_metrics(0, ma, part + nwg * 8, es == 2));
        CK(hipMemcpyAsync(host, part + nwg * 8, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, 0));
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        const auto t1 = std::chrono::steady_clock::now();
        if (i >= 5) wait_us.push_back(std::chrono::duration<float, std::micro>(t1 - t0).count());
    }
    float m[3], wv[3], wt[3];
    stats(m_us, m[0], m[1], m[2]); stats(w_us, wv[0], wv[1], wv[2]); stats(wait_us, wt[0], wt[1], wt[2]);
    const size_t rd = (size_t)w * h * es * 5 / 2;
    printf("{\"case\": \"%dx%d %d bit\", \"launches\": %zu, \"metrics_fold_us\": [%.1f, %.1f, %.1f], \"weave_us\": [%.1f, %.1f, %.1f], \"host_wait_us\": [%.1f, %.1f, %.1f], "
           "\"metrics_bytes_read\": %zu, \"metrics_GBps\": %.1f, \"workgroups\": %zu, \"S_c\": %llu, \"DB\": %llu}\n",
           w, h, depth, m_us.size(), m[0], m[1], m[2], wv[0], wv[1], wv[2], wt[0], wt[1], wt[2], rd, (double)rd / (m[0] * 1e3), nwg, host[0], host[7]);
    for (auto &f : src)
        for (auto p : f) (void)hipFree(p);
    for (auto p : dst) (void)hipFree(p);
    (void)hipFree(part); (void)hipHostFree(host);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return 0;
}

int main()
{
    if (run(720, 480, 8)) return 1;
    if (run(720, 480, 10)) return 1;
    if (run(1920, 1080, 8)) return 1;
    return run(1920, 1080, 10);
}
