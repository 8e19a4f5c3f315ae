// tools/measure_lut3d.hip — HIP-event time of one k_lut3d launch for the cases DESIGN.md §6i names (1080p 10 -> 8 bit and 2160p 10 -> 10 bit, tables of 17, 33
// and 65 points), device planes in (pseudo-random samples, so the table is read all over), a pseudo-random table, the session's plane layout out; and, as the
// yardstick, of one k_ingest_rgb launch on a 16-bit planar R'G'B' source of the same size into the same planes: step 4 of the definition alone.  5 warm-up
// launches, then 30 timed ones, each between its own pair of events; one JSON line per case with the median, the fastest, the slowest and the bytes the definition
// moves (every source sample read once, every coded sample written once; the table's bytes apart).  A measurement tool, not part of the library; it launches
// the library's own kernels through launch_lut3d and launch_ingest_rgb (csrc/device.h):
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 tools/measure_lut3d.hip -Lhevc_amd -lmihevc -Wl,-rpath,'$ORIGIN/../hevc_amd' -o build/measure_lut3d
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <functional>
#include <vector>

#include "../hevc_amd/csrc/device.h"

using namespace mihevc;

#define CK(x)                                                                              \
    do {                                                                                   \
        hipError_t e_ = (x);                                                               \
        if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } \
    } while (0)

static uint32_t g_rnd = 2463534242u;
static unsigned next_bits(int bits)
{
    g_rnd = g_rnd * 1664525u + 1013904223u;
    return (g_rnd >> 8) & ((1u << bits) - 1);
}
// n uint16 of `bits` random bits each on the device
static int random_u16(void **p, size_t n, int bits)
{
    std::vector<uint16_t> host(n);
    for (auto &v : host) v = (uint16_t)next_bits(bits);
    CK(hipMalloc(p, n * 2));
    CK(hipMemcpy(*p, host.data(), n * 2, hipMemcpyHostToDevice));
    return 0;
}
static int time_launches(const std::function<hipError_t()> &launch, std::vector<float> &us)
{
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    for (int i = 0; i < 35; i++) {
        CK(hipEventRecord(e0, 0));
        CK(launch());
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        float ms = 0;
        CK(hipEventElapsedTime(&ms, e0, e1));
        if (i >= 5) us.push_back(ms * 1000.0f);
    }
    std::sort(us.begin(), us.end());
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return 0;
}

static int run(int w, int h, int out_depth)
{
    const int pw = (w + 7) & ~7, ph = (h + 7) & ~7, B = 10;
    const size_t os = out_depth > 8 ? 2 : 1;
    const int pitch_y = (w + 15) & ~15, pitch_c = (w / 2 + 15) & ~15;
    void *yuv[3], *rgb[3], *dst[3];
    int ostride[3];
    size_t rd = 0, wr = 0;
    for (int c = 0; c < 3; c++) {
        if (random_u16(&yuv[c], (size_t)(c ? pitch_c : pitch_y) * (c ? h / 2 : h), B)) return 1;
        if (random_u16(&rgb[c], (size_t)pitch_y * h, 16)) return 1;
        rd += (size_t)(c ? w / 2 : w) * (c ? h / 2 : h) * 2;
        const int pwo = c ? pw / 2 : pw, pho = c ? ph / 2 : ph;
        ostride[c] = (pwo + 63) & ~63;
        CK(hipMalloc(&dst[c], (size_t)ostride[c] * pho * os));
        wr += (size_t)pwo * pho * os;
    }
    mihevc_rgb_format rf = {};
    rf.r = 0; rf.g = 1; rf.b = 2; rf.bit_depth = 16;
    const IngestRgbArgs ra = ingest_rgb_args(rf, 1, false, rgb[0], rgb[1], rgb[2], pitch_y, w, h, pw, ph, out_depth, dst, ostride);
    std::vector<float> base;
    if (time_launches([&] { return launch_ingest_rgb(0, ra, 0, 2, os == 2); }, base)) return 1;
    printf("{\"case\": \"k_ingest_rgb %dx%d 16 -> %d bit\", \"launches\": %zu, \"median_us\": %.1f, \"min_us\": %.1f, \"max_us\": %.1f, \"bytes_read\": %zu, \"bytes_written\": %zu, "
           "\"workgroups\": %d}\n", w, h, out_depth, base.size(), base[base.size() / 2], base.front(), base.back(), (size_t)w * h * 6, wr, ingest_rgb_workgroups(pw, ph));
    const mihevc_lut3d_src src = {B, 9, 0, {0, 0, 0, 0}};
    for (int n : {17, 33, 65}) {
        void *tab;
        const size_t entries = (size_t)n * n * n;
        if (random_u16(&tab, entries * 4, 16)) return 1;
        const Lut3dArgs a = lut3d_args(src, n, tab, yuv[0], yuv[1], yuv[2], pitch_y, pitch_c, w, h, pw, ph, out_depth, 1, false, dst, ostride);
        std::vector<float> us;
        if (time_launches([&] { return launch_lut3d(0, a, true, os == 2); }, us)) return 1;
        printf("{\"case\": \"k_lut3d %dx%d %d -> %d bit, %d points\", \"launches\": %zu, \"median_us\": %.1f, \"min_us\": %.1f, \"max_us\": %.1f, \"bytes_read\": %zu, "
               "\"bytes_written\": %zu, \"table_bytes\": %zu, \"vertex_loads\": %zu, \"workgroups\": %d, \"ratio_to_ingest_rgb\": %.2f}\n", w, h, B, out_depth, n, us.size(),
               us[us.size() / 2], us.front(), us.back(), rd, wr, entries * LUT_ENTRY_BYTES, (size_t)w * h * 4, ingest_rgb_workgroups(pw, ph),
               us[us.size() / 2] / base[base.size() / 2]);
        (void)hipFree(tab);
    }
    for (int c = 0; c < 3; c++) { (void)hipFree(yuv[c]); (void)hipFree(rgb[c]); (void)hipFree(dst[c]); }
    return 0;
}

int main()
{
    if (run(1920, 1080, 8)) return 1;
    return run(3840, 2160, 10);
}
