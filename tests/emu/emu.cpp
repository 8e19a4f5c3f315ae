// tests/emu/emu.cpp — TEST HARNESS, NOT PRODUCT.  Steps the phase programs of hevc_amd/csrc/kernels/*.h on the
// CPU with the sequential executor (one "thread" at a time, barrier = end of loop), so the kernel SOURCE can be
// checked against the oracle on machines without a GPU.  It proves the kernels' logic, not the GPU execution:
// the -m gpu tests run the real gfx950 binaries through the C ABI.  hevc_amd/ never loads this library.
// The emu_* stage entries are the twins of the mihevc_k_* entries (device.hip) and build the same argument blocks (csrc/stage_args.h); those
// that take a mihevc_cost_params take a last argument sign_hide as well (CostParams::sign_hide).  emu_transform_sdh / emu_transform4_sdh are
// the twins of mihevc_k_transform_sdh; the picture hash twin is in pichash.cpp.
#include <chrono>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../hevc_amd/csrc/stage_args.h"

using namespace mihevc;

// LDS is not zeroed on the device: with EMU_SHARED_FILL=<seed> the shared state of every workgroup starts as pseudo-random bytes, so a
// read of a field the program never initialised shows up as a mismatch against the oracle (default: zeros)
static int emu_order() { const char *e = getenv("EMU_ORDER"); return e ? atoi(e) : 0; }
template <class S> using Shared = std::unique_ptr<S, void (*)(void *)>;
template <class S> static Shared<S> fresh_shared()
{
    S *p = (S *)malloc(sizeof(S));
    const char *e = getenv("EMU_SHARED_FILL");
    if (!e) { memset((void *)p, 0, sizeof(S)); return Shared<S>(p, free); }
    static unsigned long long x = 0;
    if (!x) x = 0x9E3779B97F4A7C15ull ^ (unsigned long long)atoll(e);
    unsigned char *b = (unsigned char *)p;
    for (size_t i = 0; i < sizeof(S); i++) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; b[i] = (unsigned char)(x >> 32); }
    return Shared<S>(p, free);
}

// views of the three caller planes (Y, Cb, Cr) of a picture w samples wide, unpadded, from row y0 on (chroma: row y0 / 2)
template <typename T> struct Views {
    Plane<T> p[3];
    template <class V> Views(V *const *pl, int w, int y0 = 0)
    {
        for (int i = 0; i < 3; i++) { const int s = i ? w / 2 : w; p[i] = {(T *)pl[i] + (ptrdiff_t)(i ? y0 / 2 : y0) * s, s}; }
    }
};

// a reference picture copied into planes with the device's borders (PAD_Y / PAD_C), border extended
template <typename T> struct PaddedPicture {
    std::vector<T> buf[3];
    Plane<const T> p[3];
    PaddedPicture(const void *const *src, int w, int h)
    {
        for (int i = 0; i < 3; i++) {
            const int pw = i ? w / 2 : w, ph = i ? h / 2 : h, pad = i ? PAD_C : PAD_Y, stride = pw + 2 * pad;
            buf[i].assign((size_t)stride * (ph + 2 * pad), 0);
            const Plane<T> pl{buf[i].data() + (size_t)pad * stride + pad, stride};
            for (int y = 0; y < ph; y++) memcpy(pl.p + (ptrdiff_t)y * stride, (const T *)src[i] + (size_t)y * pw, pw * sizeof(T));
            for (int k = 0; k < pad_border_count(pw, ph, pad); k++) pad_border_sample<T>(pl, pw, ph, pad, k);
            p[i] = {pl.p, stride};
        }
    }
};

// ---- EMU_WAVES=<seed>: the four waves of a workgroup as four host threads -------------------------------------------------------------
// The sequential executor runs the code BETWEEN two phases once, so it cannot see a wave that reads shared state for a uniform branch
// after another wave has already entered the next phase and rewritten it (the NxN race of round 1).  Here every wave runs the whole CTU
// program on its own thread, phases end in a real barrier, and a random wave is delayed after each barrier to provoke such skew.  A wave
// that takes a different branch misses a barrier: the barrier times out and the frame call reports -2.
struct WaveBarrier {       // spinning barrier on C++ atomics (sanitizers follow their acquire / release edges)
    std::atomic<int> waiting{0}, generation{0};
    std::atomic<bool> broken{false};
    bool wait()
    {
        if (broken.load()) return false;
        const int gen = generation.load(std::memory_order_acquire);
        if (waiting.fetch_add(1, std::memory_order_acq_rel) + 1 == NT / 64) {
            waiting.store(0, std::memory_order_relaxed);
            generation.fetch_add(1, std::memory_order_release);
            return true;
        }
        const auto t0 = std::chrono::steady_clock::now();
        while (generation.load(std::memory_order_acquire) == gen) {
            if (broken.load()) return false;
            if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(3)) { broken.store(true); return false; }
            std::this_thread::yield();
        }
        return true;
    }
};
struct WaveAbort {};
struct WaveExec {
    int wave;
    WaveBarrier *bar;
    unsigned long long rnd;
    template <class F> void lanes(F &&f) { for (int l = 0; l < 64; l++) f(wave * 64 + l); }
    template <class F> void phase(F &&f)
    {
        lanes(f);
        if (!bar->wait()) throw WaveAbort{};
        rnd ^= rnd << 13; rnd ^= rnd >> 7; rnd ^= rnd << 17;
        if ((rnd >> 40) % 16 == 0) std::this_thread::sleep_for(std::chrono::microseconds(30));      // this wave falls behind
    }
    template <class F> void wave_step(F &&f) { lanes(f); }
    void atomic_add(int *p, int v) { __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
    void atomic_add(unsigned *p, unsigned v) { __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
    void atomic_add(unsigned long long *p, unsigned long long v) { __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
    void atomic_or(unsigned *p, unsigned v) { __atomic_fetch_or(p, v, __ATOMIC_RELAXED); }
    void atomic_and(unsigned *p, unsigned v) { __atomic_fetch_and(p, v, __ATOMIC_RELAXED); }
    void atomic_min(unsigned long long *p, unsigned long long v)
    {
        unsigned long long cur = __atomic_load_n(p, __ATOMIC_RELAXED);
        while (v < cur && !__atomic_compare_exchange_n(p, &cur, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    }
    unsigned long long peek(const unsigned long long *p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
    void atomic_add_global(unsigned long long *p, unsigned long long v) { __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
};
// run one workgroup program on four wave threads; false when a barrier broke
template <class Program> static bool run_waves(unsigned long long seed, Program &&program)
{
    static WaveBarrier bar;        // one long-lived object (workgroups run one after the other): sanitizers track a mutex by its address
    bar.waiting.store(0); bar.broken.store(false);
    std::vector<std::thread> th;
    for (int wv = 0; wv < NT / 64; wv++)
        th.emplace_back([&, wv] {
            WaveExec ex{wv, &bar, (seed + 1) * 0x9E3779B97F4A7C15ull + (unsigned long long)wv * 0xD1B54A32D192ED03ull};
            try { program(ex); } catch (const WaveAbort &) {}
        });
    for (auto &t : th) t.join();
    return !bar.broken.load();
}


// Runs one workgroup program, program(ex), per call: on the sequential executor (EMU_ORDER: its thread order; one executor for every workgroup of
// the picture), or with EMU_WAVES=<seed> on four wave threads seeded with seed + salt.  false: a barrier broke, and the frame call reports -2
struct Stepper {
    SeqExec seq;
    const char *waves = getenv("EMU_WAVES");
    Stepper() { seq.order = emu_order(); }
    template <class Program> bool operator()(unsigned salt, Program &&program)
    {
        if (waves) return run_waves((unsigned long long)atoll(waves) + salt, program);
        program(seq);
        return true;
    }
};

// A P picture (f1 == nullptr) against the reference f0, or a B picture between the anchors f0 (list 0) and f1 (list 1), in the order of the
// device's launches (device.hip stage_inter): P: search centres (prm.pre_search without centres0), list-0 search, P CTU program, intra second pass
// (prm.intra_in_p); B: list-0 and list-1 searches, B CTU program
template <typename T>
static int inter_frame(const void *const *s, const void *const *f0, const void *const *f1, int w, int h, const CostParams &prm, const int16_t *centers0,
                       const int16_t *centers1, void *const *o, mihevc_cu_rec *cu, int16_t *const *coef, int32_t *me_dump0, int32_t *me_dump1, unsigned long long *est)
{
    const bool b = f1 != nullptr;
    const int nref = b ? 2 : 1, n_ctu = ctus_of(w) * ctus_of(h), R = prm.me_range;
    const bool pre = !b && prm.pre_search && !centers0;
    PaddedPicture<T> ref0(f0, w, h);
    std::unique_ptr<PaddedPicture<T>> ref1(b ? new PaddedPicture<T>(f1, w, h) : nullptr);
    std::vector<int32_t> me[2];
    for (int l = 0; l < nref; l++) me[l].resize((size_t)n_ctu * 63);
    std::vector<int16_t> cen(pre ? (size_t)n_ctu * 2 : 0, 0);
    std::vector<IpInfo> ipv(!b && prm.intra_in_p ? (size_t)n_ctu : 0, IpInfo{0, 0, 0});
    if (est) *est = 0;
    const InterArgs<T> a = inter_args<T>(Views<const T>(s, w).p, ref0.p, b ? ref1->p : nullptr, Views<T>(o, w).p, w, h, prm, AnalysisOut{cu, {coef[0], coef[1], coef[2]}, est},
                                         pre ? cen.data() : centers0, centers1, me[0].data(), me[1].data(), ipv.empty() ? nullptr : ipv.data());
    Stepper step;
    if (pre) {
        std::vector<uint8_t> ls((size_t)(w / 4) * (h / 4), 0), lr = ls;
        const PreArgs<T> pa = pre_args<T>(a, ls.data(), lr.data(), cen.data());
        for (int i = 0; i < 2 * (w / 4) * (h / 4); i++) lowres_sample<T>(pa, i);
        for (int c = 0; c < n_ctu; c++) {
            PreShared ps;
            if (!step(31u * (unsigned)c, [&](auto &ex) { pre_search_program<T>(ex, ps, pa, c); })) return -2;
        }
    }
    std::vector<uint8_t> win((size_t)me_win_elems(R) + 8);
    std::vector<T> wy(mc_win_y_bytes<T>(R) / sizeof(T)), wu(mc_win_c_bytes<T>(R) / sizeof(T)), wv(wu.size());
    for (int list = 0; list < nref; list++) {
        const InterArgs<T> al = list ? list1_view(a) : a;
        for (int c = 0; c < n_ctu; c++) {
            Shared<MeShared<T>> ms = fresh_shared<MeShared<T>>();
            if (!step((unsigned)c + 1000u * list, [&](auto &ex) { me_search_program<T>(ex, *ms, win.data(), al, c); })) return -2;
        }
    }
    int32_t *me_dump[2] = {me_dump0, me_dump1};
    for (int l = 0; l < nref; l++)
        if (me_dump[l]) memcpy(me_dump[l], me[l].data(), me[l].size() * sizeof(int32_t));
    for (int c = 0; c < n_ctu; c++) {
        Shared<InterShared<T>> is = fresh_shared<InterShared<T>>();
        Shared<BiShared> bs = b ? fresh_shared<BiShared>() : Shared<BiShared>(nullptr, free);
        if (!step(7919u * (unsigned)c, [&](auto &ex) {
                using Ex = std::remove_reference_t<decltype(ex)>;
                if (b) inter_ctu_program<T, Ex, true>(ex, *is, wy.data(), wu.data(), wv.data(), a, c, bs.get());
                else inter_ctu_program<T>(ex, *is, wy.data(), wu.data(), wv.data(), a, c);
            }))
            return -2;
    }
    if (a.ip) {       // intra second pass, two rounds like the device's two launches
        const IntraArgs<T> ia = intra_in_p_args(a);
        for (int round = 0; round < 2; round++)
            for (int c = 0; c < n_ctu; c++) {
                if (!ip_eligible(ia.ip, ia.ctus_w, ia.ctus_h, c % ia.ctus_w, c / ia.ctus_w, round)) continue;
                Shared<IntraShared<T>> is = fresh_shared<IntraShared<T>>();
                if (!step(104729u * (unsigned)c, [&](auto &ex) { intra_ctu_program<T>(ex, *is, ia, c % ia.ctus_w, c / ia.ctus_w); })) return -2;
            }
    }
    return 0;
}

template <typename T>
static int intra_frame(const void *const *s, int w, int h, const CostParams &prm, void *const *o, mihevc_cu_rec *cu, int16_t *const *coef, unsigned long long *est)
{
    IntraArgs<T> a = intra_args<T>(Views<const T>(s, w).p, Views<T>(o, w).p, w, h, prm, AnalysisOut{cu, {coef[0], coef[1], coef[2]}, est});
    if (est) *est = 0;
    Stepper step;
    // same launch order as the device: per tile, one anti-diagonal (cx + 2 cy inside the tile) at a time
    const int tcn = a.prm.tile_cols > 1 ? a.prm.tile_cols : 1, trn = a.prm.tile_rows > 1 ? a.prm.tile_rows : 1;
    const int colw = (a.ctus_w + tcn - 1) / tcn, rowh = (a.ctus_h + trn - 1) / trn;
    for (int d = 0; d <= (colw - 1) + 2 * (rowh - 1); d++) {
        a.diagonal = d;
        for (int b = 0; b < tcn * trn * rowh; b++) {
            const int tile = b / rowh, r = b % rowh, tx = tile % tcn, ty = tile / tcn;
            const int cx0 = tile_bd(tx, tcn, a.ctus_w), cx1 = tile_bd(tx + 1, tcn, a.ctus_w), cy0 = tile_bd(ty, trn, a.ctus_h), cy1 = tile_bd(ty + 1, trn, a.ctus_h);
            const int cyi = cy0 + r, cxi = cx0 + d - 2 * r;
            if (cyi >= cy1 || cxi < cx0 || cxi >= cx1) continue;
            Shared<IntraShared<T>> is = fresh_shared<IntraShared<T>>();
            if (!step((unsigned)(cyi * 4096 + cxi), [&](auto &ex) { intra_ctu_program<T>(ex, *is, a, cxi, cyi); })) return -2;
        }
    }
    return 0;
}

// stage A alone, every CTU in raster order: the twin of mihevc_k_intra_plan
template <typename T> static int intra_plan(const void *const *s, int w, int h, const CostParams &prm, mihevc_intra_plan *plan)
{
    const Plane<T> none[3]{};
    static_assert(sizeof(IntraPlan) == sizeof(mihevc_intra_plan), "mihevc_intra_plan is IntraPlan");
    const int n_ctu = ctus_of(w) * ctus_of(h);
    memset(plan, 0, (size_t)n_ctu * sizeof *plan);
    const IntraArgs<T> a = intra_args<T>(Views<const T>(s, w).p, none, w, h, prm, AnalysisOut{nullptr, {nullptr, nullptr, nullptr}, nullptr}, (IntraPlan *)plan);
    Stepper step;
    for (int c = 0; c < n_ctu; c++) {
        Shared<IntraShared<T>> is = fresh_shared<IntraShared<T>>();
        if (!step(211u * (unsigned)c, [&](auto &ex) { intra_plan_program<T>(ex, *is, a, c % a.ctus_w, c / a.ctus_w); })) return -2;
    }
    intra_plan_clear_unwritten(plan, w, h);
    return 0;
}

// row0 / y_org: deblock rows [row0, row0 + h) of a whole picture's planes as a picture of its own whose first y_org rows belong to the slice above
// (DeblockArgs::y_org; the band extended by the rows its neighbours hand over, csrc/slice_group.h)
template <typename T> static int deblock(void *const *r, int w, int h, const mihevc_cu_rec *cu, int bit_depth, int row0 = 0, int y_org = 0)
{
    for (int dir = 0; dir < 2; dir++) {
        const DeblockArgs<T> a = deblock_args<T>(Views<T>(r, w, row0).p, w, h, cu + (ptrdiff_t)(row0 / 8) * (w / 8), bit_depth, dir, y_org);
        for (int i = 0; i < (w / 8) * (h / 8) * 2; i++) deblock_segment<T>(a, i);
    }
    return 0;
}

// y0 / halo: the planes are those of a whole picture of which rows [y0, y0 + h) are coded here as one slice whose filters run across the seams
// (SaoArgs::halo; csrc/slice_group.h): the kernel then sees its band as the picture and finds the neighbour rows where the exchange puts them
template <typename T>
static int sao(const void *const *s, const void *const *d, int w, int h, const CostParams &prm, void *const *o, mihevc_sao_ctu *out, int y0 = 0, int halo = 0,
               uint32_t *sse_ctu = nullptr, const mihevc_cu_rec *cu = nullptr)
{
    const SaoArgs<T> a = sao_args<T>(Views<const T>(s, w, y0).p, Views<const T>(d, w, y0).p, Views<T>(o, w, y0).p, w, h, prm, out,
                                     cu ? cu + (size_t)(y0 / 8) * (w / 8) : nullptr, halo, sse_ctu);
    Stepper step;
    for (int c = 0; c < ctus_of(w) * ctus_of(h); c++) {
        SaoShared<T> ss;
        if (!step(131u * (unsigned)c, [&](auto &ex) { sao_ctu_program<T>(ex, ss, a, c); })) return -2;
    }
    return 0;          // the CTU programs applied the offsets themselves (as k_sao_decide does)
}

extern "C" {
int emu_inter_frame(const void *sy, const void *su, const void *sv, const void *ry, const void *ru, const void *rv, int w, int h, const mihevc_cost_params *prm,
                    const int16_t *centers, void *oy, void *ou, void *ov, mihevc_cu_rec *cu, int16_t *cy, int16_t *cu_, int16_t *cv, int32_t *me_dump,
                    unsigned long long *est, int sign_hide)
{
    const void *s[3] = {sy, su, sv}, *f[3] = {ry, ru, rv};
    void *o[3] = {oy, ou, ov};
    int16_t *c[3] = {cy, cu_, cv};
    return with_depth(prm->bit_depth, [&](auto t) {
        return inter_frame<decltype(t)>(s, f, nullptr, w, h, cost_params_of(*prm, sign_hide), centers, nullptr, o, cu, c, me_dump, nullptr, est);
    });
}
int emu_b_frame(const void *sy, const void *su, const void *sv, const void *r0y, const void *r0u, const void *r0v, const void *r1y, const void *r1u, const void *r1v,
                int w, int h, const mihevc_cost_params *prm, const int16_t *centers0, const int16_t *centers1, void *oy, void *ou, void *ov, mihevc_cu_rec *cu,
                int16_t *cy, int16_t *cu_, int16_t *cv, int32_t *me_dump0, int32_t *me_dump1, unsigned long long *est, int sign_hide)
{
    const void *s[3] = {sy, su, sv}, *f0[3] = {r0y, r0u, r0v}, *f1[3] = {r1y, r1u, r1v};
    void *o[3] = {oy, ou, ov};
    int16_t *c[3] = {cy, cu_, cv};
    return with_depth(prm->bit_depth, [&](auto t) {
        return inter_frame<decltype(t)>(s, f0, f1, w, h, cost_params_of(*prm, sign_hide), centers0, centers1, o, cu, c, me_dump0, me_dump1, est);
    });
}
int emu_intra_frame(const void *sy, const void *su, const void *sv, int w, int h, const mihevc_cost_params *prm, void *oy, void *ou, void *ov,
                    mihevc_cu_rec *cu, int16_t *cy, int16_t *cu_, int16_t *cv, unsigned long long *est, int sign_hide)
{
    const void *s[3] = {sy, su, sv};
    void *o[3] = {oy, ou, ov};
    int16_t *c[3] = {cy, cu_, cv};
    return with_depth(prm->bit_depth, [&](auto t) { return intra_frame<decltype(t)>(s, w, h, cost_params_of(*prm, sign_hide), o, cu, c, est); });
}
int emu_intra_plan(const void *sy, const void *su, const void *sv, int w, int h, const mihevc_cost_params *prm, mihevc_intra_plan *plan, int sign_hide)
{
    if (prm->tile_cols > ctus_of(w) || prm->tile_rows > ctus_of(h)) return MIHEVC_EINVAL;
    const void *s[3] = {sy, su, sv};
    return with_depth(prm->bit_depth, [&](auto t) { return intra_plan<decltype(t)>(s, w, h, cost_params_of(*prm, sign_hide), plan); });
}
int emu_deblock(void *y, void *u, void *v, int w, int h, const mihevc_cu_rec *cu, int bit_depth)
{
    void *r[3] = {y, u, v};
    return with_depth(bit_depth, [&](auto t) { return deblock<decltype(t)>(r, w, h, cu, bit_depth); });
}
int emu_deblock_band(void *y, void *u, void *v, int w, int row0, int h, int y_org, const mihevc_cu_rec *cu, int bit_depth)
{
    void *r[3] = {y, u, v};
    return with_depth(bit_depth, [&](auto t) { return deblock<decltype(t)>(r, w, h, cu, bit_depth, row0, y_org); });
}
int emu_sao(const void *sy, const void *su, const void *sv, const void *dy, const void *du, const void *dv, int w, int h, const mihevc_cost_params *prm,
            void *oy, void *ou, void *ov, mihevc_sao_ctu *out, int sign_hide)
{
    const void *s[3] = {sy, su, sv}, *d[3] = {dy, du, dv};
    void *o[3] = {oy, ou, ov};
    return with_depth(prm->bit_depth, [&](auto t) { return sao<decltype(t)>(s, d, w, h, cost_params_of(*prm, sign_hide), o, out); });
}
int emu_sao_band(const void *sy, const void *su, const void *sv, const void *dy, const void *du, const void *dv, int w, int y0, int h, int halo,
                 const mihevc_cost_params *prm, void *oy, void *ou, void *ov, mihevc_sao_ctu *out, int sign_hide)
{
    const void *s[3] = {sy, su, sv}, *d[3] = {dy, du, dv};
    void *o[3] = {oy, ou, ov};
    return with_depth(prm->bit_depth, [&](auto t) { return sao<decltype(t)>(s, d, w, h, cost_params_of(*prm, sign_hide), o, out, y0, halo); });
}
// the fused loop filter (SaoArgs::cu): r* = the PRE-deblock reconstruction; y0 / h / halo as emu_sao_band (cu: the whole picture's records)
int emu_loop_filter(const void *sy, const void *su, const void *sv, const void *ry, const void *ru, const void *rv, int w, int y0, int h, int halo, const mihevc_cu_rec *cu,
                    const mihevc_cost_params *prm, void *oy, void *ou, void *ov, mihevc_sao_ctu *out, int sign_hide)
{
    const void *s[3] = {sy, su, sv}, *r[3] = {ry, ru, rv};
    void *o[3] = {oy, ou, ov};
    return with_depth(prm->bit_depth, [&](auto t) { return sao<decltype(t)>(s, r, w, h, cost_params_of(*prm, sign_hide), o, out, y0, halo, nullptr, cu); });
}
int emu_sao_sse(const void *sy, const void *su, const void *sv, const void *dy, const void *du, const void *dv, int w, int h, const mihevc_cost_params *prm,
                void *oy, void *ou, void *ov, mihevc_sao_ctu *out, uint32_t *sse_ctu, int sign_hide)
{
    const void *s[3] = {sy, su, sv}, *d[3] = {dy, du, dv};
    void *o[3] = {oy, ou, ov};
    return with_depth(prm->bit_depth, [&](auto t) { return sao<decltype(t)>(s, d, w, h, cost_params_of(*prm, sign_hide), o, out, 0, 0, sse_ctu); });
}

// K3 on n_blocks blocks of 2^log2n (log2n 3..5: luma TUs of a pseudo-CTU, log2n 2: 4x4 DCT blocks in its chroma planes), every block in scan
// `scan`, with sign data hiding when sign_hide
int emu_transform_sdh(const int16_t *res, int16_t *lvl, int16_t *rec, int n_blocks, int log2n, int qp, int bit_depth, int intra, int scan, int sign_hide)
{
    if (log2n < 2 || log2n > 5 || scan < 0 || scan > 2) return -3;
    const int n = 1 << log2n, lt = log2n < 3 ? 3 : log2n, per = log2n == 2 ? 32 : 1024 >> (2 * log2n);       // blocks per pseudo-CTU
    // block b of a pseudo-CTU -> index of its top-left sample in the 1536-sample arrays
    auto origin = [&](int b) {
        if (log2n > 2) return (b / (32 >> log2n)) * n * 32 + (b % (32 >> log2n)) * n;
        return 1024 + (b >> 4) * 256 + ((b & 15) >> 2) * 4 * 16 + (b & 3) * 4;
    };
    SeqExec ex;
    for (int first = 0; first < n_blocks; first += per) {
        Shared<ResidualShared> s = fresh_shared<ResidualShared>();
        residual_init(ex, *s);
        ex.phase([&](int tid) {
            if (tid < 16) {
                const int blk = log2n > 2 ? first + ((tid >> 2) * 8 >> lt) * (32 >> lt) + ((tid & 3) * 8 >> lt) : first + tid;
                s->tu_log2[tid] = blk < n_blocks ? (uint8_t)lt : 0;
                s->tu_intra[tid] = (uint8_t)intra;
            }
            for (int i = tid; i < 1536; i += NT) s->res[i] = 0;
        });
        ex.phase([&](int tid) {
            for (int b = tid; b < per; b += NT) {
                if (first + b >= n_blocks) continue;
                const int o = origin(b), st = o < 1024 ? 32 : 16;
                for (int k = 0; k < n * n; k++) s->res[o + (k / n) * st + k % n] = res[(size_t)(first + b) * n * n + k];
            }
        });
        ex.phase([&](int tid) { for (int i = tid; i < 1536; i += NT) { SampleLoc l = locate(*s, i); l.scan = scan; s->desc[i] = pack_loc(l); } });
        residual_pipeline(ex, *s, qp, qp, bit_depth, whole_ctu(), 0, sign_hide);
        for (int b = 0; b < per && first + b < n_blocks; b++) {
            const int o = origin(b), st = o < 1024 ? 32 : 16;
            for (int k = 0; k < n * n; k++) {
                lvl[(size_t)(first + b) * n * n + k] = s->lvl[o + (k / n) * st + k % n];
                rec[(size_t)(first + b) * n * n + k] = s->res[o + (k / n) * st + k % n];
            }
        }
    }
    return 0;
}

// k_transform4_blocks on n_blocks 4x4 blocks (DST-VII when dst, else DCT), the same grid of NT / 16 blocks per workgroup
int emu_transform4_sdh(const int16_t *res, int16_t *lvl, int16_t *rec, int n_blocks, int qp, int bit_depth, int intra, int dst, int scan, int sign_hide)
{
    if (scan < 0 || scan > 2) return -3;
    SeqExec ex;
    for (int first = 0; first < n_blocks; first += NT / 16) {
        Shared<Transform4Shared> s = fresh_shared<Transform4Shared>();
        transform4_program(ex, *s, res, lvl, rec, n_blocks, first, qp, bit_depth, intra, dst, scan, sign_hide);
    }
    return 0;
}
}
