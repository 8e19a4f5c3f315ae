// tools/measure_sr_yuv.hip — HIP-event times of what the Y'CbCr sources and the target sizes add to the learned super-resolution path, beside
// tools/measure_sr.hip and with its method (warm-up launches, then timed ones, each between its own pair of events; median, fastest, slowest):
//   1  k_sr_from_yuv alone at 480x270 and 960x540 sources, 8 and 10 bit, scale 4 and 2: 5 warm-up launches, 30 timed, with the bytes it moves and the GB/s
//   2  the two launches of the resized route, k_ingest_rgb into the 10-bit intermediate picture and k_scale into 8-bit session planes, each alone and as a pair:
//      3416x1920 -> 1920x1080 (a 854x480 source through x4), 2560x1440 -> 1920x1080 (1280x720 through x2), 5120x2880 -> 3840x2160 (1280x720 through x4)
//   3  one whole B = 6 frame from a Y'CbCr source, every launch of the entry: 480x270 -> 1920x1080 on the direct route against 854x480 -> 1920x1080 on the
//      resized route (3 warm-up frames, 10 timed), and of the second the share of k_sr_from_yuv and of the two launches behind the network
// Gaussian weights and random pictures.  One JSON line per measurement.  A measurement tool, not part of the library; it launches the library's own kernels
// through csrc/device.h:
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 tools/measure_sr_yuv.hip -Lhevc_amd -lmihevc -Wl,-rpath,'$ORIGIN/../hevc_amd' -o build/measure_sr_yuv
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

#include "../hevc_amd/csrc/device.h"
#include "../hevc_amd/csrc/scale_taps.h"

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

static uint32_t g_rnd = 2463534242u;
static float uni() { g_rnd ^= g_rnd << 13; g_rnd ^= g_rnd >> 17; g_rnd ^= g_rnd << 5; return (float)(g_rnd >> 8) / 16777216.0f; }

// a random planar 4:2:0 picture on the device: tight rows, the three planes one behind the other
struct Yuv {
    uint8_t *d = nullptr;
    const void *p[3];
    int alloc(int w, int h, int depth)
    {
        const size_t es = depth > 8 ? 2 : 1, n = (size_t)w * h * 3 / 2;
        std::vector<uint8_t> pic(n * es);
        for (size_t i = 0; i < n; i++) {
            const unsigned v = (unsigned)(uni() * (float)(1 << depth));
            if (es == 2) { pic[2 * i] = (uint8_t)v; pic[2 * i + 1] = (uint8_t)(v >> 8); }
            else pic[i] = (uint8_t)v;
        }
        CK(hipMalloc(&d, pic.size())); CK(hipMemcpy(d, pic.data(), pic.size(), hipMemcpyHostToDevice));
        p[0] = d; p[1] = d + (size_t)w * h * es; p[2] = d + (size_t)w * h * es * 5 / 4;
        return 0;
    }
    ~Yuv() { (void)hipFree(d); }
};
// 4:2:0 planes of a coded size with aligned strides, TO-byte samples
struct Planes {
    uint8_t *d = nullptr;
    void *p[3];
    int stride[3], pw, ph;
    int alloc(int w, int h, size_t es)
    {
        pw = (w + 7) & ~7; ph = (h + 7) & ~7;
        size_t off[3], n = 0;
        for (int c = 0; c < 3; c++) { stride[c] = ((c ? pw / 2 : pw) + 15) & ~15; off[c] = n; n += ((size_t)stride[c] * (c ? ph / 2 : ph) * es + 255) & ~(size_t)255; }
        CK(hipMalloc(&d, n));
        for (int c = 0; c < 3; c++) p[c] = d + off[c];
        return 0;
    }
    ~Planes() { (void)hipFree(d); }
};
// the scale tables of nw x nh -> w x h on the device
struct TapSet {
    ScaleBlock blk;
    uint8_t *d = nullptr;
    const int32_t *first[4];
    const int16_t *coef[4];
    int build(int nw, int nh, int w, int h)
    {
        if (!scale_block_build(nw, nh, w, h, SC_TH, SC_ROWS, blk)) return 1;
        CK(hipMalloc(&d, blk.bytes.size())); CK(hipMemcpy(d, blk.bytes.data(), blk.bytes.size(), hipMemcpyHostToDevice));
        tap_pointers(d, blk.first, first); tap_pointers(d, blk.coef, coef);
        return 0;
    }
    ~TapSet() { (void)hipFree(d); }
};

static int input_alone(int sw, int sh, int depth, int scale)
{
    Yuv src;
    if (src.alloc(sw, sh, depth)) return 1;
    const size_t halves = (size_t)sw * sh * SR_CIN0 / (scale == 2 ? 4 : 1);
    uint16_t *x;
    CK(hipMalloc(&x, halves * 2));
    const mihevc_sr_yuv f = {sw, sh, depth, 6, 0, {0, 0, 0}};
    const SrYuvArgs a = sr_yuv_args(f, scale, src.p[0], src.p[1], src.p[2], sw, sw / 2, x);
    float us[3];
    if (timed([&] { return launch_sr_from_yuv(0, a, depth > 8); }, 5, 30, us)) return 1;
    const double bytes = (double)halves * 2 + (double)sw * sh * 3 / 2 * (depth > 8 ? 2 : 1);
    printf("{\"case\": \"k_sr_from_yuv x%d %dx%d %d bit\", \"median_us\": %.1f, \"min_us\": %.1f, \"max_us\": %.1f, \"mbytes\": %.1f, \"gb_per_s\": %.0f, \"workgroups\": %d}\n",
           scale, sw, sh, depth, us[0], us[1], us[2], bytes / 1e6, bytes / us[0] * 1e-3, sr_yuv_workgroups(sw, sh));
    (void)hipFree(x);
    return 0;
}

// k_ingest_rgb of three half planes nw x nh into the 10-bit intermediate picture, k_scale into w x h at 8 bit
static int resized_pair(int nw, int nh, int w, int h)
{
    std::vector<uint16_t> half((size_t)3 * nw * nh);
    for (auto &v : half) v = (uint16_t)(0x3000 + (unsigned)(uni() * 2048.0f));      // halves between 0.125 and 0.5
    uint16_t *o;
    CK(hipMalloc(&o, half.size() * 2)); CK(hipMemcpy(o, half.data(), half.size() * 2, hipMemcpyHostToDevice));
    Planes mid, dst;
    TapSet tab;
    if (mid.alloc(nw, nh, 2) || dst.alloc(w, h, 1) || tab.build(nw, nh, w, h)) return 1;
    const mihevc_rgb_format halves = {0, 0, 1, 2, 1, 0, 0, 0, {0, 0, 0, 0}};
    const IngestRgbArgs ia = ingest_rgb_args(halves, 1, false, o, o + (size_t)nw * nh, o + (size_t)2 * nw * nh, nw, nw, nh, mid.pw, mid.ph, 10, mid.p, mid.stride);
    const ScaleArgs sa = scale_args(10, mid.p[0], mid.p[1], mid.p[2], mid.stride[0], mid.stride[1], nw, nh, w, h, dst.pw, dst.ph, 8, dst.p, dst.stride, tab.first, tab.coef, tab.blk.taps);
    float a[3], b[3], c[3];
    if (timed([&] { return launch_ingest_rgb(0, ia, 1, 2, true); }, 5, 30, a)) return 1;
    if (timed([&] { return launch_scale(0, sa, true, false); }, 5, 30, b)) return 1;
    if (timed([&] { hipError_t e = launch_ingest_rgb(0, ia, 1, 2, true); return e != hipSuccess ? e : launch_scale(0, sa, true, false); }, 5, 30, c)) return 1;
    printf("{\"case\": \"resized route %dx%d -> %dx%d\", \"k_ingest_rgb_us\": %.1f, \"k_scale_us\": %.1f, \"pair_median_us\": %.1f, \"pair_min_us\": %.1f, \"pair_max_us\": %.1f}\n",
           nw, nh, w, h, a[0], b[0], c[0], c[1], c[2]);
    (void)hipFree(o);
    return 0;
}

// a whole frame of the entry from a Y'CbCr source of sw x sh through a x4 network of `blocks` into a w x h session at 8 bit
static int whole_frame(int blocks, int sw, int sh, int w, int h)
{
    const size_t count = sr_net_count(4, blocks);
    std::vector<float> wt(count);
    for (auto &v : wt) v = 0.02f * std::sqrt(-2.0f * std::log(uni() + 1e-7f)) * std::cos(6.2831853f * uni());
    SrNet net;
    if (!sr_net_build(4, blocks, wt.data(), count, net)) return 1;
    size_t off[SR_BUFS];
    const size_t bytes = sr_arena_layout(sw, sh, off);
    uint8_t *arena;
    uint16_t *dw;
    float *db;
    CK(hipMalloc(&arena, bytes)); CK(hipMemset(arena, 0, bytes));
    CK(hipMalloc(&dw, net.wpk.size() * 2)); CK(hipMemcpy(dw, net.wpk.data(), net.wpk.size() * 2, hipMemcpyHostToDevice));
    CK(hipMalloc(&db, net.bias.size() * 4)); CK(hipMemcpy(db, net.bias.data(), net.bias.size() * 4, hipMemcpyHostToDevice));
    Yuv src;
    if (src.alloc(sw, sh, 8)) return 1;
    const int nw = 4 * sw, nh = 4 * sh;
    const bool resized = nw != w || nh != h;
    Planes mid, dst;
    TapSet tab;
    if (dst.alloc(w, h, 1) || (resized && (mid.alloc(nw, nh, 2) || tab.build(nw, nh, w, h)))) return 1;
    const mihevc_sr_yuv f = {sw, sh, 8, 6, 0, {0, 0, 0}};
    const SrYuvArgs ya = sr_yuv_args(f, 4, src.p[0], src.p[1], src.p[2], sw, sw / 2, (uint16_t *)(arena + off[SR_X]));
    const mihevc_rgb_format halves = {0, 0, 1, 2, 1, 0, 0, 0, {0, 0, 0, 0}};
    const uint16_t *o = (const uint16_t *)(arena + off[SR_OUT]);
    const IngestRgbArgs direct = ingest_rgb_args(halves, 1, false, o, o + (size_t)nw * nh, o + (size_t)2 * nw * nh, nw, nw, nh, dst.pw, dst.ph, 8, dst.p, dst.stride);
    IngestRgbArgs ia = direct;
    ScaleArgs sa = {};
    if (resized) {
        ia = ingest_rgb_args(halves, 1, false, o, o + (size_t)nw * nh, o + (size_t)2 * nw * nh, nw, nw, nh, mid.pw, mid.ph, 10, mid.p, mid.stride);
        sa = scale_args(10, mid.p[0], mid.p[1], mid.p[2], mid.stride[0], mid.stride[1], nw, nh, w, h, dst.pw, dst.ph, 8, dst.p, dst.stride, tab.first, tab.coef, tab.blk.taps);
    }
    auto tail = [&]() -> hipError_t {
        if (!resized) return launch_ingest_rgb(0, direct, 1, 2, false);
        hipError_t e = launch_ingest_rgb(0, ia, 1, 2, true);
        return e != hipSuccess ? e : launch_scale(0, sa, true, false);
    };
    auto frame = [&]() -> hipError_t {
        hipError_t e = launch_sr_from_yuv(0, ya, false);
        if (e == hipSuccess) e = launch_sr_network(0, net, arena, dw, db, sw, sh);
        return e != hipSuccess ? e : tail();
    };
    float us[3], in[3], tl[3];
    if (timed(frame, 3, 10, us)) return 1;
    if (timed([&] { return launch_sr_from_yuv(0, ya, false); }, 5, 30, in)) return 1;
    if (timed(tail, 5, 30, tl)) return 1;
    printf("{\"case\": \"frame x4 B=%d yuv420p %dx%d -> %dx%d (%s)\", \"median_ms\": %.2f, \"min_ms\": %.2f, \"max_ms\": %.2f, \"k_sr_from_yuv_us\": %.1f, "
           "\"behind_the_network_us\": %.1f, \"share_of_frame\": %.4f, \"arena_mb\": %.0f}\n",
           blocks, sw, sh, w, h, resized ? "resized" : "direct", us[0] / 1000, us[1] / 1000, us[2] / 1000, in[0], tl[0], (in[0] + tl[0]) / us[0], bytes / 1048576.0);
    (void)hipFree(arena); (void)hipFree(dw); (void)hipFree(db);
    return 0;
}

int main()
{
    for (int size = 0; size < 2; size++)
        for (int depth : {8, 10})
            for (int scale : {4, 2})
                if (input_alone(size ? 960 : 480, size ? 540 : 270, depth, scale)) return 1;
    if (resized_pair(3416, 1920, 1920, 1080) || resized_pair(2560, 1440, 1920, 1080) || resized_pair(5120, 2880, 3840, 2160)) return 1;
    if (whole_frame(6, 480, 270, 1920, 1080) || whole_frame(6, 854, 480, 1920, 1080)) return 1;
    return 0;
}
