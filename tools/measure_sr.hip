// tools/measure_sr.hip — HIP-event times of the learned super-resolution path: for an x4 RRDBNet at 480x270 and 960x540 sources, every distinct
// layer shape of the network as one k_sr_conv launch (5 warm-up launches, then 30 timed ones, each between its own pair of events; median, fastest, slowest,
// and the achieved TFLOP/s of the real multiply-adds against the 2.5 PFLOP/s the MFMA issue rate implies), then the whole frame (k_sr_input and every launch;
// 3 warm-up runs, 10 timed) for 23 and for 6 blocks.  Gaussian weights and a random picture: zero operands would read high.  One JSON line per measurement.
// `measure_sr layers` times only the 64 -> 32 and 192 -> 64 layers at 960x540: what a counter pass of its own is run over.  A measurement tool, not part of the
// library; it launches the library's own kernels through launch_sr_conv / launch_sr_input / launch_sr_network (csrc/device.h) over the list of csrc/sr_net.h:
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 tools/measure_sr.hip -Lhevc_amd -lmihevc -Wl,-rpath,'$ORIGIN/../hevc_amd' -o build/measure_sr
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <set>
#include <tuple>
#include <vector>

#include "../hevc_amd/csrc/device.h"

using namespace mihevc;

#define CK(x)                                                                              \
    do {                                                                                   \
        hipError_t e_ = (x);                                                               \
        if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } \
    } while (0)

// median, fastest and slowest of `n` launches after `warm` warm-up ones, in microseconds
static int timed(const std::function<hipError_t()> &launch, int warm, int n, float (&us3)[3])
{
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    std::vector<float> us;
    for (int i = 0; i < warm + n; i++) {
        CK(hipEventRecord(e0, 0));
        CK(launch());
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        float ms = 0;
        CK(hipEventElapsedTime(&ms, e0, e1));
        if (i >= warm) us.push_back(ms * 1000.0f);
    }
    std::sort(us.begin(), us.end());
    us3[0] = us[us.size() / 2]; us3[1] = us.front(); us3[2] = us.back();
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return 0;
}

static int run(int blocks, int sw, int sh, bool per_layer, bool whole, bool two_only)
{
    const size_t count = sr_net_count(4, blocks);
    std::vector<float> w(count);
    uint32_t rnd = 2463534242u;
    auto uni = [&]() { rnd ^= rnd << 13; rnd ^= rnd >> 17; rnd ^= rnd << 5; return (float)(rnd >> 8) / 16777216.0f; };
    for (auto &v : w) v = 0.02f * std::sqrt(-2.0f * std::log(uni() + 1e-7f)) * std::cos(6.2831853f * uni());
    SrNet net;
    if (!sr_net_build(4, blocks, w.data(), count, net)) return 1;
    size_t off[SR_BUFS];
    const size_t bytes = sr_arena_layout(sw, sh, off);
    uint8_t *arena, *src;
    uint16_t *dw;
    float *db;
    CK(hipMalloc(&arena, bytes));
    CK(hipMemset(arena, 0, bytes));
    CK(hipMalloc(&dw, net.wpk.size() * 2)); CK(hipMemcpy(dw, net.wpk.data(), net.wpk.size() * 2, hipMemcpyHostToDevice));
    CK(hipMalloc(&db, net.bias.size() * 4)); CK(hipMemcpy(db, net.bias.data(), net.bias.size() * 4, hipMemcpyHostToDevice));
    std::vector<uint8_t> pic((size_t)3 * sw * sh);
    for (auto &b : pic) b = (uint8_t)(uni() * 256.0f);
    CK(hipMalloc(&src, pic.size())); CK(hipMemcpy(src, pic.data(), pic.size(), hipMemcpyHostToDevice));
    const mihevc_rgb_format fmt = {0, 0, 1, 2, 0, 8, 0, 0, {0, 0, 0, 0}};
    const void *planes[3] = {src, src + (size_t)sw * sh, src + (size_t)2 * sw * sh};
    const SrInputArgs ia = sr_input_args(fmt, 4, sw, sh, planes, sw, (uint16_t *)(arena + off[SR_X]));
    // one whole frame first: every buffer then holds what the network leaves there
    CK(launch_sr_input(0, ia, 0, 1));
    CK(launch_sr_network(0, net, arena, dw, db, sw, sh));
    CK(hipDeviceSynchronize());
    float us[3];
    if (per_layer) {
        std::set<std::tuple<int, int, int, int>> seen;
        for (const SrLaunch &l : net.launches) {
            const SrLayer &y = net.layers[(size_t)l.layer];
            if (!seen.insert({y.cin_pad, y.cout_pad, l.level, l.up}).second) continue;
            if (two_only && !((y.cin_pad == 64 && y.cout_pad == 32) || (y.cin_pad == 192 && y.cout_pad == 64))) continue;
            const SrConvArgs a = sr_launch_args(net, l, arena, dw, db, sw, sh, 0.2f);
            if (timed([&] { return launch_sr_conv(0, a, y.cin_pad, y.cout_pad, l.planar != 0); }, 5, 30, us)) return 1;
            const double flop = 2.0 * 9 * y.cin * y.cout * (double)a.w * a.h;
            printf("{\"case\": \"k_sr_conv %d -> %d at %dx%d%s\", \"median_us\": %.1f, \"min_us\": %.1f, \"max_us\": %.1f, \"tflops\": %.1f, \"of_2500\": %.3f, \"workgroups\": %d}\n",
                   y.cin, y.cout, a.w, a.h, l.up ? " (enlarging)" : "", us[0], us[1], us[2], flop / us[0] * 1e-6, flop / us[0] * 1e-6 / 2500.0, sr_conv_workgroups(a.w, a.h));
        }
    }
    if (whole) {
        if (timed([&] { hipError_t e = launch_sr_input(0, ia, 0, 1); return e != hipSuccess ? e : launch_sr_network(0, net, arena, dw, db, sw, sh); }, 3, 10, us)) return 1;
        double flop = 0;
        for (const SrLaunch &l : net.launches) flop += 2.0 * 9 * net.layers[(size_t)l.layer].cin * net.layers[(size_t)l.layer].cout * (double)(sw << l.level) * (sh << l.level);
        printf("{\"case\": \"network x4 B=%d %dx%d -> %dx%d\", \"median_ms\": %.2f, \"min_ms\": %.2f, \"max_ms\": %.2f, \"tflops\": %.1f, \"launches\": %zu, \"arena_mb\": %.0f}\n",
               blocks, sw, sh, 4 * sw, 4 * sh, us[0] / 1000, us[1] / 1000, us[2] / 1000, flop / us[0] * 1e-6, net.launches.size() + 1, bytes / 1048576.0);
    }
    (void)hipFree(arena); (void)hipFree(dw); (void)hipFree(db); (void)hipFree(src);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "layers")) return run(1, 960, 540, true, false, true);
    for (int size = 0; size < 2; size++) {
        const int sw = size ? 960 : 480, sh = size ? 540 : 270;
        if (run(1, sw, sh, true, false, false)) return 1;
        for (int blocks : {6, 23})
            if (run(blocks, sw, sh, false, true, false)) return 1;
    }
    return 0;
}
