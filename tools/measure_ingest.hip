// tools/measure_ingest.hip — HIP-event time of one k_ingest launch at 1920x1080 for the two sources DESIGN.md §6c names, device planes in, the session's plane
// layout out: 5 warm-up launches, then 30 timed ones, each between its own pair of events; one JSON line per case with the median, the fastest, the slowest and
// the bytes the definition moves.  A measurement tool, not part of the library; it launches the library's own kernel through launch_ingest (csrc/device.h):
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 tools/measure_ingest.hip -Lhevc_amd -lmihevc -Wl,-rpath,'$ORIGIN/../hevc_amd' -o build/measure_ingest
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <vector>

#include "../hevc_amd/csrc/device.h"

using namespace mihevc;

#define CK(x)                                                                              \
    do {                                                                                   \
        hipError_t e_ = (x);                                                               \
        if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } \
    } while (0)

static int run(const char *name, mihevc_src_format f, int out_depth)
{
    const int w = 1920, h = 1080, pw = (w + 7) & ~7, ph = (h + 7) & ~7;
    const size_t es = f.bit_depth > 8 ? 2 : 1, eo = out_depth > 8 ? 2 : 1;
    void *src[3] = {nullptr, nullptr, nullptr}, *dst[3];
    int ostride[3];
    size_t rd = 0, wr = 0;
    const int pitch_c = (src_chroma_row(f, w) + 15) & ~15;
    for (int c = 0; c < (f.semi_planar ? 2 : 3); c++) {
        const size_t bytes = (size_t)(c ? pitch_c : w) * (c ? src_chroma_rows(f, h) : h) * es;
        CK(hipMalloc(&src[c], bytes));
        CK(hipMemset(src[c], 0x5A, bytes));
        rd += (size_t)(c ? src_chroma_row(f, w) : w) * (c ? src_chroma_rows(f, h) : h) * es;
    }
    for (int c = 0; c < 3; c++) {
        const int pwo = c ? pw / 2 : pw, pho = c ? ph / 2 : ph;
        ostride[c] = (pwo + 63) & ~63;
        CK(hipMalloc(&dst[c], (size_t)ostride[c] * pho * eo));
        wr += (size_t)pwo * pho * eo;
    }
    const IngestArgs a = ingest_args(f, src[0], src[1], src[2], w, pitch_c, w, h, pw, ph, out_depth, dst, ostride);
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    std::vector<float> us;
    for (int i = 0; i < 35; i++) {
        CK(hipEventRecord(e0, 0));
        CK(launch_ingest(0, a, es == 2, eo == 2));
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        float ms = 0;
        CK(hipEventElapsedTime(&ms, e0, e1));
        if (i >= 5) us.push_back(ms * 1000.0f);
    }
    std::sort(us.begin(), us.end());
    printf("{\"case\": \"%s -> 4:2:0 %d bit, 1920x1080\", \"launches\": %zu, \"median_us\": %.1f, \"min_us\": %.1f, \"max_us\": %.1f, \"bytes_read\": %zu, \"bytes_written\": %zu, \"align\": [%d, %d]}\n",
           name, out_depth, us.size(), us[us.size() / 2], us.front(), us.back(), rd, wr, a.align[0], a.align[1]);
    for (auto p : src) if (p) (void)hipFree(p);
    for (auto p : dst) (void)hipFree(p);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return 0;
}

int main()
{
    if (run("yuv422p10le", mihevc_src_format{422, 0, 10, 0, {0, 0, 0, 0}}, 10)) return 1;
    return run("yuv444p16le", mihevc_src_format{444, 0, 16, 0, {0, 0, 0, 0}}, 10);
}
