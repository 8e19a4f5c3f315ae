// hevc_amd/csrc/session.cpp — the encoder session behind mihevc_open / send_frame / receive_packet.
//
// Pipeline: source pictures are collected in HBM; every `gops_in_flight * keyint` pictures
// (or at flush) the chunk is encoded.  Closed GOPs are independent, so the chunk's GOPs run in LOCK-STEP: step t
// launches each stage once for picture t of every GOP (blockIdx.y = GOP lane).  Per step: intra anti-diagonals
// (t = 0) or ME + inter CTU (t > 0) -> deblock V/H -> SAO decide/apply -> border pad -> SSE, then one D2H copy of
// the step's symbols into pinned memory on a second stream, and one CABAC job per picture on the host pool.
// The device never waits for CABAC except when the 4-deep symbol ring wraps.
// Replaces, for the selected files, the `ffmpeg -c:v libx265` child of the reference (core/transcoder.py:506).
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <thread>

#include "md5.h"
#include "session.h"

constexpr int kSeamRows = 8;      // rows of the pre-deblock reconstruction exchanged either side of a seam (deblocking reads 4 and writes 3; one 8x8 grid row)

// the session's one failure path: every later call returns fail_code, and the other slices of the picture stop waiting for this one
int fail(mihevc_session *s, std::string msg)
{
    { std::lock_guard<std::mutex> l(s->m); s->err = std::move(msg); }
    s->failed = true;
    if (s->group) s->group->fail();
    return MIHEVC_EDEVICE;
}

// padded 0: a plain picture; 1: a reference picture with its PAD border all round; 2: a work picture with kSeamRows rows above and below (the rows the
// neighbour slices hand over for deblocking across seams; unused otherwise)
int alloc_planes(mihevc_session *s, CachedBlock<uint8_t> mem[3], void *p[3], int stride[3], int padded)
{
    for (int i = 0; i < 3; i++) {
        int w = i ? s->w / 2 : s->w, h = i ? s->h / 2 : s->h, pad = padded == 1 ? (i ? PAD_C : PAD_Y) : 0, vm = padded == 2 ? (i ? kSeamRows / 2 : kSeamRows) : pad;
        stride[i] = (w + 2 * pad + 63) & ~63;
        HIPCK(s, mem[i].alloc(s->device, (size_t)stride[i] * (h + 2 * vm) * esize(s), false));
        p[i] = mem[i] + ((size_t)vm * stride[i] + pad) * esize(s);
    }
    return 0;
}

namespace {

// symbol block of one picture: [cu | coef Y | coef U | coef V | sao | sse[3] | rate estimate | hash[3] | ssim[3]]; the device twin carries the per-CTU squared errors
// behind it (SaoArgs::sse_ctu: never copied to the host, k_sse_fold turns them into sse[3]).  hash: the CRC / checksum words of cfg.pic_hash 2 / 3 (k_pic_hash_fold);
// ssim: the int64 sums of cfg.ssim (k_ssim_fold).  Both sit in the 256 bytes that begin at sse: the block is no larger for them
struct SymLayout {
    size_t cu, cu_bytes, cy, cu_, cv, sao, sse, est, hash, ssim, total, sse_ctu, dev_total;
    SymLayout(int w, int h)
    {
        size_t n8 = (size_t)(w / 8) * (h / 8), ny = (size_t)w * h, nctu = (size_t)((w + 31) / 32) * ((h + 31) / 32);
        const size_t row = (size_t)(w / 8) * sizeof(mihevc_cu_rec);
        auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
        cu = al(row);                 // one row of records in front of the picture's and one behind: where the neighbour slices' rows go (slice_group.h)
        cu_bytes = n8 * sizeof(mihevc_cu_rec);
        cy = al(cu + cu_bytes + row);
        cu_ = al(cy + ny * 2);
        cv = al(cu_ + ny / 2);
        sao = al(cv + ny / 2);
        sse = al(sao + nctu * sizeof(mihevc_sao_ctu));
        est = sse + 3 * sizeof(unsigned long long);
        hash = est + sizeof(unsigned long long);
        ssim = (hash + 3 * sizeof(uint32_t) + 7) & ~(size_t)7;
        total = al(ssim + 3 * sizeof(long long));
        sse_ctu = total;
        dev_total = al(sse_ctu + nctu * 3 * sizeof(uint32_t));
    }
};

// sessions this process has open on a device.  A chunk runs as lane groups only while its session is the device's only one: a second session's launches already
// fill the first one's launch tails, and with the process's four hardware queues two sessions of five busy streams each had their uploads and copies queue
// behind kernels (bench.py's two-session leg from pinned host buffers: -5 %).  The stream does not depend on the choice.
std::atomic<int> &open_sessions(int device) { static std::atomic<int> n[64]; return n[device & 63]; }
long long ssim_window_count(const mihevc_session *s, int c) { return (long long)ssim_windows_x(c ? s->w / 2 : s->w) * ssim_windows_y(c ? s->h / 2 : s->h); }
size_t md5_pic_bytes(const mihevc_session *s) { return (size_t)s->w * s->h * 3 / 2 * esize(s); }

// (a failure midway: the local lane gives back what it had taken)
int ensure_lanes(mihevc_session *s, int n)
{
    SymLayout sl(s->w, s->h);
    while ((int)s->lane.size() < n) {
        mihevc_session::Lane L;
        for (int k = 0; k < (s->cfg.bframes != 0 ? 3 : 2); k++)
            if (int e = alloc_planes(s, L.rec_mem[k], L.rec_p[k], L.rec_stride, 1)) return e;
        if (int e = alloc_planes(s, L.work_mem, L.work_p, L.work_stride, 2)) return e;
        HIPCK(s, L.me.alloc(s->device, (size_t)s->n_ctu * 63 * sizeof(int32_t), false));
        if (s->cfg.bframes != 0) HIPCK(s, L.me1.alloc(s->device, (size_t)s->n_ctu * 63 * sizeof(int32_t), false));
        HIPCK(s, L.ip.alloc(s->device, (size_t)s->n_ctu * sizeof(IpInfo), false));
        HIPCK(s, L.plan.alloc(s->device, (size_t)s->n_ctu * sizeof(IntraPlan), false));
        for (int k = 0; k < s->ring; k++) {
            HIPCK(s, L.sym_dev[k].alloc(s->device, sl.dev_total, false));
            HIPCK(s, L.sym_host[k].alloc(s->device, sl.total, true));
            if (s->cfg.pic_hash == 1) HIPCK(s, L.md5_host[k].alloc(s->device, md5_pic_bytes(s), true));
        }
        s->lane.push_back(std::move(L));
    }
    return 0;
}

// grow a cached buffer to at least `need` bytes, rounded up with `round_mask` (the next session's chunk then finds a block of the same size in the cache)
int grow(mihevc_session *s, CachedBuf &b, size_t need, size_t round_mask, bool with_host)
{
    if (need <= b.d.bytes()) return 0;
    b.d.reset(); b.h.reset();
    const size_t cap = (need + round_mask) & ~round_mask;
    HIPCK(s, b.d.alloc(s->device, cap, false));
    if (with_host) HIPCK(s, b.h.alloc(s->device, cap, true));
    return 0;
}
// argument blocks of one lock-step step: five arrays of `gops` entries each, so one launch per stage covers all lanes
template <typename T> struct StepLayout {
    size_t intra, inter, dbk_v, dbk_h, sao, total;
    explicit StepLayout(int gops)
    {
        auto al = [](size_t v) { return (v + 63) & ~(size_t)63; };
        intra = 0;
        inter = al(intra + (size_t)2 * gops * sizeof(IntraArgs<T>));      // [gops, 2 gops): the IDR re-analysis pass, compacted
        dbk_v = al(inter + gops * sizeof(InterArgs<T>));
        dbk_h = al(dbk_v + gops * sizeof(DeblockArgs<T>));
        sao = al(dbk_h + gops * sizeof(DeblockArgs<T>));
        total = al(sao + gops * sizeof(SaoArgs<T>));
    }
};
template <typename T> struct StepView {
    IntraArgs<T> *intra; InterArgs<T> *inter; DeblockArgs<T> *dbk_v, *dbk_h; SaoArgs<T> *sao;
    StepView(uint8_t *base, const StepLayout<T> &l, int t, int first = 0)      // first: entry the view begins at (a lane group's part of the arrays)
    {
        uint8_t *b = base + (size_t)t * l.total;
        intra = (IntraArgs<T> *)(b + l.intra) + first; inter = (InterArgs<T> *)(b + l.inter) + first;
        dbk_v = (DeblockArgs<T> *)(b + l.dbk_v) + first; dbk_h = (DeblockArgs<T> *)(b + l.dbk_h) + first; sao = (SaoArgs<T> *)(b + l.sao) + first;
    }
};

template <typename T> Plane<T> mk(void *p, int stride) { return Plane<T>{(T *)p, stride}; }
template <typename T> Plane<const T> mkc(void *p, int stride) { return Plane<const T>{(const T *)p, stride}; }

// CABAC of one picture: `parts` host jobs share its tiles (cfg.p_tiles / the IDR grid: every tile is its own substream), the last one to finish
// puts the access unit together and publishes the packet.  One part = the whole picture in one job, as before round 3.
struct PictureJob {
    mihevc_session *s;
    int grp, slot, lane_i, slice_type, poc, qp, prev_gop_len, parts, n_tiles, dec_pos;      // poc: place in the GOP in display order, dec_pos: in decoding order
    int64_t index, pts, dts, dec_index;      // index: display order (frame records, reconstructions); dec_index: decoding order (packets)
    bool first_of_stream, reorder;      // reorder: the stream announces B pictures (dts one frame early, output delay in the picture timing SEI)
    PictureSyms pic;
    std::vector<std::vector<uint8_t>> sub;
    std::atomic<int> left;
    std::atomic<long long> ns{0};
    std::mutex err_m;
    std::string err;        // first refusal of any part (encode_tiles)
    uint8_t md5[3][16];     // cfg.pic_hash 1: written by the job's MD5 part
};

void picture_symbols(mihevc_session *s, int slot, int lane_i, PictureSyms &pic)
{
    SymLayout sl(s->w, s->h);
    const uint8_t *b = s->lane[lane_i].sym_host[slot];
    pic.cu = (const mihevc_cu_rec *)(b + sl.cu);
    pic.coef[0] = (const int16_t *)(b + sl.cy); pic.coef[1] = (const int16_t *)(b + sl.cu_); pic.coef[2] = (const int16_t *)(b + sl.cv);
    pic.sao = s->cfg.sao ? (const mihevc_sao_ctu *)(b + sl.sao) : nullptr;
}

// last part of a picture: access unit = AUD first (7.4.2.4.4), parameter sets (+ HDR10 SEI), buffering period at the IDR, picture timing, the slice
void publish_picture(PictureJob *j)
{
    mihevc_session *s = j->s;
    auto t0 = std::chrono::steady_clock::now();
    SymLayout sl(s->w, s->h);
    const uint8_t *b = s->lane[j->lane_i].sym_host[j->slot];
    Packet pk;
    pk.pts = j->pts; pk.dts = j->dts; pk.key = j->slice_type == 2;
    pk.error = j->err;      // (every part has finished: no lock needed)
    // a picture's later slices (sessions on other devices, cfg.slice_index > 0) contribute their slice NAL unit only: the access unit's
    // delimiter, parameter sets and SEI come with slice 0
    const bool au_head = s->cfg.slice_count <= 1 || s->cfg.slice_index == 0;
    if (s->cfg.aud && au_head) write_aud(j->slice_type, pk.data);
    if (au_head && j->slice_type == 2 && (j->first_of_stream || s->cfg.repeat_headers)) pk.data.insert(pk.data.end(), s->headers.begin(), s->headers.end());
    if (s->cfg.hrd && au_head) {
        if (j->slice_type == 2) write_sei_buffering_period(s->cfg, pk.data);
        // clock ticks since the previous buffering period: position in the GOP, or the previous GOP's length at an IDR
        // (cfg.bframes: removal happens in decoding order; a picture is shown one tick after the picture at its display place was removed)
        write_sei_pic_timing(s->cfg, (uint32_t)(j->dec_pos > 0 ? j->dec_pos - 1 : (j->dec_index > 0 ? j->prev_gop_len - 1 : 0)), pk.data,
                             j->reorder ? (uint32_t)(j->poc + 1 - j->dec_pos) : 0u);
    }
    assemble_picture(s->cfg, j->pic, j->sub, pk.data, false);
    // decoded picture hash: a suffix SEI behind the slice (cfg.pic_hash 1 MD5 from the job's MD5 part, 2 / 3 the device's words in the symbol block)
    if (s->cfg.pic_hash) write_sei_picture_hash(s->cfg, s->cfg.pic_hash - 1, s->cfg.pic_hash == 1 ? (const void *)j->md5 : (const void *)(b + sl.hash), pk.data);
    const unsigned long long *sse = (const unsigned long long *)(b + sl.sse);
    pk.ready = true;
    auto t1 = std::chrono::steady_clock::now();
    s->entropy_ns += j->ns.load() + std::chrono::duration_cast<std::chrono::nanoseconds>(t1 - t0).count();
    const int grp = j->grp, slot = j->slot;
    const int64_t index = j->index;
    {
        std::lock_guard<std::mutex> l(s->m);
        s->stats.sse_y += (double)sse[0]; s->stats.sse_u += (double)sse[1]; s->stats.sse_v += (double)sse[2];
        if ((size_t)index < s->quality.size()) {
            auto &q = s->quality[(size_t)index];
            const long long *sq = (const long long *)(b + sl.ssim);
            for (int c = 0; c < 3; c++) {
                q.sse[c] = sse[c];
                q.ssim[c] = s->cfg.ssim ? sq[c] : 0;
                s->ssim_total[c] += q.ssim[c];
            }
            q.known = true;
        }
        s->stats.bytes_out += (int64_t)pk.data.size();
        if ((size_t)index < s->frames.size()) {
            auto &fr = s->frames[(size_t)index];
            fr.bits_local = (long long)pk.data.size() * 8;
            fr.est_local = *(const unsigned long long *)(b + sl.est);
            if (!s->group) {          // (slices with one rate plan: the step loop sums sizes and estimates over the slices at fixed points)
                fr.bits = fr.bits_local;
                fr.est_q4 = *(const unsigned long long *)(b + sl.est);
                fr.est_known = true;
            }
        }
        s->packets[j->dec_index] = std::move(pk);
        s->frames_done++;
        delete j;
        s->slot[grp][slot].jobs_open--;
        s->cv.notify_all();      // under the lock: mihevc_close may delete the session as soon as its last job has let go of the mutex
    }
}

void entropy_part(PictureJob *j, int part)
{
    auto t0 = std::chrono::steady_clock::now();
    const int t_a = (int)((long long)j->n_tiles * part / j->parts), t_b = (int)((long long)j->n_tiles * (part + 1) / j->parts);
    std::string err;
    encode_tiles(j->s->cfg, j->pic, t_a, t_b, j->sub, &err);
    if (!err.empty()) { std::lock_guard<std::mutex> l(j->err_m); if (j->err.empty()) j->err = "picture " + std::to_string(j->index) + ": " + err; }
    j->ns += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
    if (j->left.fetch_sub(1) == 1) publish_picture(j);
}

// cfg.pic_hash 1: MD5 of the picture's three components from the pinned copy of the final reconstruction, beside the CABAC parts of its job
void md5_part(PictureJob *j)
{
    mihevc_session *s = j->s;
    auto t0 = std::chrono::steady_clock::now();
    const uint8_t *p = s->lane[j->lane_i].md5_host[j->slot];
    const size_t es = esize(s);
    for (int c = 0; c < 3; c++) {
        const size_t row = (size_t)(c ? s->w / 2 : s->w) * es;
        const int rows = c ? s->h / 2 : s->h;
        md5_plane(p, row, row, rows, j->md5[c]);
        p += row * rows;
    }
    j->ns += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
    if (j->left.fetch_sub(1) == 1) publish_picture(j);
}

// sum of |a - b| over every 4th sample of every 4th row of consecutive pending source pictures: out[i] for the pair (i - 1, i), out[0] = 0
template <typename T> int scene_differences(mihevc_session *s, int n, std::vector<unsigned long long> &out)
{
    const size_t in_bytes = (size_t)n * sizeof(ScenePic<T>), need = ((in_bytes + 255) & ~(size_t)255) + (size_t)n * sizeof(unsigned long long);
    if (int e = grow(s, s->scene, need, 0xfff, false)) return e;
    std::vector<ScenePic<T>> pics((size_t)n);
    for (int i = 0; i < n; i++) pics[(size_t)i] = ScenePic<T>{(const T *)s->pending[(size_t)i].p[0], s->pending[(size_t)i].stride[0]};
    unsigned long long *d_out = (unsigned long long *)((uint8_t *)s->scene.d + ((in_bytes + 255) & ~(size_t)255));
    HIPCK(s, hipMemcpyAsync(s->scene.d, pics.data(), in_bytes, hipMemcpyHostToDevice, s->st_compute));
    HIPCK(s, hipMemsetAsync(d_out, 0, (size_t)n * sizeof(unsigned long long), s->st_compute));
    HIPCK(s, launch_scene_diff<T>(s->st_compute, (const ScenePic<T> *)s->scene.d.get(), d_out, s->w, s->h, n));
    HIPCK(s, hipMemcpyAsync(out.data(), d_out, (size_t)n * sizeof(unsigned long long), hipMemcpyDeviceToHost, s->st_compute));
    HIPCK(s, hipStreamSynchronize(s->st_compute));
    return 0;
}

// ---- the slices of one picture exchange rows (cfg.slice_halo; csrc/slice_group.h) ------------------------------------------------------------
// job tables of one step: [export: lanes x 8][import: lanes x 8][pull: lanes x 3 x reach], RowCopy each
struct JobLayout {
    int lanes, reach;
    size_t exp, imp, pull, total;
    JobLayout(int lanes_, int reach_) : lanes(lanes_), reach(reach_)
    {
        exp = 0; imp = exp + (size_t)lanes * 8 * sizeof(RowCopy); pull = imp + (size_t)lanes * 8 * sizeof(RowCopy);
        total = (pull + (size_t)lanes * 3 * (size_t)std::max(1, reach) * sizeof(RowCopy) + 255) & ~(size_t)255;
    }
};

constexpr const char *kPeerFailed = "another slice of the picture failed";

static int group_sum(mihevc_session *s, std::vector<double> &v)
{
    if (!s->group) return 0;
    if (!s->group->allreduce(v)) return fail(s, kPeerFailed);
    return 0;
}

// cfg.bframes = -1: are B pictures worth it for this chunk?  With a B picture between every two anchors an anchor predicts from TWO pictures back; that pays when
// motion stays trackable over two pictures (translation, static content) and costs when it does not (zoom, fades: tools/rd_curve.py, profiles/r03: +7 % bits on
// the `stress` clip even with B pictures at the anchors' QP).  The probe asks the integer search itself: for up to 4 pictures spread over the chunk, k_me_search
// of the SOURCE picture against the source one place back and two places back (copied into lane 0's reference buffers, border padded); c1 / c2 = the 32x32 nodes'
// best costs (SAD << 4 + lambda * mvd bits) summed over all CTUs.  B pictures when c2 <= kProbeRatio x c1.  A 1/4-size search cannot tell (sub-sample
// motion dominates its SADs: it rated the translating clip WORSE than the zooming one).  ~0.4 ms per chunk at 1080p.  stats.reserved[0] / [1] keep the last
// c1 / c2 per CTU, [2] the decision (tests and tools read them).
constexpr double kProbeRatio = 1.4;
template <typename T> static int probe_bframes(mihevc_session *s, int n, bool &use_b)
{
    use_b = false;
    if (n < 3) return 0;
    if (int e = ensure_lanes(s, 1)) return e;
    mihevc_session::Lane &L = s->lane[0];
    const int K = std::min(4, (n - 2 + 15) / 16 + 1);
    std::vector<int> at;
    for (int k = 0; k < K; k++) { const int p = 2 + (int)((long long)(n - 3) * k / std::max(1, K - 1)); if (at.empty() || at.back() != p) at.push_back(p); }
    const size_t o_inter = (2 * sizeof(SaoArgs<T>) + 255) & ~(size_t)255, o_total = o_inter + 2 * at.size() * sizeof(InterArgs<T>);
    if (int e = grow(s, s->probe, o_total, 0xffff, false)) return e;
    uint8_t *base = (uint8_t *)s->probe.d;
    mihevc_cost_params c;
    mihevc_cost_params_for_qp(s->qp_p, s->cfg.bit_depth, s->me_range, &c);
    const CostParams P{c.qp, c.qp_c, c.bit_depth, c.lambda_sad_q4, c.lambda_q4, c.me_range, 1, 1, false, false, false, false, false, false, false, 0};
    SaoArgs<T> pad[2];
    memset(pad, 0, sizeof pad);
    for (int k = 0; k < 2; k++) { for (int i = 0; i < 3; i++) pad[k].out[i] = mk<T>(L.rec_p[k][i], L.rec_stride[i]); pad[k].w = s->w; pad[k].h = s->h; }
    std::vector<InterArgs<T>> ia(2 * at.size());
    for (size_t k = 0; k < at.size(); k++)
        for (int d = 0; d < 2; d++) {
            InterArgs<T> &a = ia[2 * k + (size_t)d];
            memset((void *)&a, 0, sizeof a);
            const Src &src = s->pending[(size_t)at[k]];
            for (int i = 0; i < 3; i++) { a.src[i] = mkc<T>(src.p[i], src.stride[i]); a.ref[i] = mkc<T>(L.rec_p[d][i], L.rec_stride[i]); }
            a.w = s->w; a.h = s->h; a.ctus_w = s->ctus_w; a.prm = P; a.me = d ? L.me1 : L.me;
        }
    HIPCK(s, hipMemcpyAsync(base, pad, sizeof pad, hipMemcpyHostToDevice, s->st_compute));
    HIPCK(s, hipMemcpyAsync(base + o_inter, ia.data(), ia.size() * sizeof(InterArgs<T>), hipMemcpyHostToDevice, s->st_compute));
    std::vector<int32_t> me((size_t)2 * at.size() * s->n_ctu * 63);
    const size_t es = esize(s), me_bytes = (size_t)s->n_ctu * 63 * sizeof(int32_t);
    for (size_t k = 0; k < at.size(); k++) {
        for (int d = 0; d < 2; d++) {          // the luma of the pictures one and two places back -> the reference buffers (the search reads luma only)
            const Src &r = s->pending[(size_t)(at[k] - 1 - d)];
            HIPCK(s, hipMemcpy2DAsync(L.rec_p[d][0], L.rec_stride[0] * es, r.p[0], r.stride[0] * es, s->w * es, s->h, hipMemcpyDeviceToDevice, s->st_compute));
        }
        HIPCK(s, launch_pad<T>(s->st_compute, (const SaoArgs<T> *)base, s->w, s->h, 2));
        for (int d = 0; d < 2; d++) {
            HIPCK(s, launch_me_search<T>(s->st_compute, (const InterArgs<T> *)(base + o_inter) + 2 * k + (size_t)d, s->n_ctu, 1, s->me_range, 0));
            HIPCK(s, hipMemcpyAsync(me.data() + (2 * k + (size_t)d) * s->n_ctu * 63, d ? L.me1 : L.me, me_bytes, hipMemcpyDeviceToHost, s->st_compute));
        }
    }
    HIPCK(s, hipStreamSynchronize(s->st_compute));
    unsigned long long c1 = 0, c2 = 0;
    for (size_t k = 0; k < at.size(); k++)
        for (int ctu = 0; ctu < s->n_ctu; ctu++) {
            // node 0 (the 32x32 block); CTUs the picture cuts off have no such node: their four 16x16 / sixteen 8x8 nodes stand in
            for (int d = 0; d < 2; d++) {
                const int32_t *m = me.data() + ((2 * k + (size_t)d) * s->n_ctu + (size_t)ctu) * 63;
                unsigned long long v = 0;
                if (m[2] >= 0) v = (unsigned long long)m[2];
                else for (int nd = 1; nd < 21; nd++) { if (nd < 5 ? m[3 * nd + 2] >= 0 : m[3 * (1 + ((nd - 5) >> 2)) + 2] < 0 && m[3 * nd + 2] >= 0) v += (unsigned long long)m[3 * nd + 2]; }
                (d ? c2 : c1) += v;
            }
        }
    use_b = (double)c2 <= kProbeRatio * (double)c1;
    const unsigned long long per = (unsigned long long)s->n_ctu * at.size();
    s->stats.reserved[0] = (int32_t)std::min<unsigned long long>(0x7fffffff, c1 / per);
    s->stats.reserved[1] = (int32_t)std::min<unsigned long long>(0x7fffffff, c2 / per);
    s->stats.reserved[2] = use_b;
    return 0;
}

// ---- one chunk ------------------------------------------------------------------------------------------------------------------------------------
// the slices of one picture exchange rows (cfg.slice_halo; csrc/slice_group.h): the bands in reach and the chunk's row-copy job tables
struct Halo {
    bool on = false;
    int up = 0, dn = 0, top = 0, bottom = 0, reach = 0;      // a neighbour above / below; rows in reach above / below; bands in reach
    std::vector<std::pair<int, int>> reach_up, reach_dn;
    JobLayout jl{0, 0};
    uint8_t *hj = nullptr, *dj = nullptr;
    const RowCopy *jobs(int t, size_t part) const { return (const RowCopy *)(dj + (size_t)t * jl.total + part); }
};

// the lanes one launch sequence covers at a step: their entries in the step's argument arrays are [base, base + n), `lanes` in that order.  Step 0 is one part
// of all lanes in lane order (base 0; Chunk::at places them)
struct Part {
    int grp = 0, base = 0, n = 0;
    std::vector<int> lanes;
    hipStream_t st = nullptr;
};

template <typename T> struct Chunk {
    const int n, gops, steps, ring;
    const int64_t first_index;                    // output index of pending[0]
    const GopLayout gl; const SymLayout sl; const StepLayout<T> lay;
    const size_t flat_off;                        // the pre-search blocks: behind every step's block and one for the rho trial
    bool bf = false;                              // B pictures in this chunk (cfg.bframes; -1: the probe decides)
    int n_pre = 0;                                // pre-search blocks: one per picture of the chunk (stream order); with B pictures a second one per picture for list 1
    size_t need = 0, low_pic = 0;
    uint8_t *ha = nullptr, *da = nullptr, *low = nullptr; int16_t *cen = nullptr;      // argument blocks (host staging, device), pre-search pictures and centres
    Halo halo;
    // Lane groups.  From step 1 on the lanes of a step run as `groups` independent launch sequences, each on its own stream: group 0 the even lanes on the
    // compute stream, group 1 the odd lanes on st_pre.  Lanes are sorted longest GOP first and the active ones are a prefix, so alternating keeps the groups
    // within one lane of each other as GOPs run out.  Every step's argument arrays hold group 0's lanes first, then group 1's: a group's launch is
    // (array + group_base, group_size).
    // The stream does not depend on `groups`: across lanes nothing is shared from step 1 on (pictures, tables, symbol blocks and frame records are per lane),
    // and RateControl::decide_p reads only its own lane's records at fixed lags: CABAC sizes of steps <= t - (ring - 1), estimates of steps <= t - 2.  rho_pi,
    // ratio_*, beta_bp and the budgets are constants of the chunk once step 0 is over.  Each group keeps those lags in its own steps (the wait for the
    // slot's CABAC jobs, the wait for the symbol copy of step t - 2), so every lane sees the same inputs whichever group it is in.
    int groups = 1;
    int group_size(int grp, int t) const { const int B = gl.batch[(size_t)t]; return groups == 1 ? (grp ? 0 : B) : (B + 1 - grp) / 2; }
    int group_base(int grp, int t) const { return grp ? group_size(0, t) : 0; }
    int at(int t, int g) const { return groups == 1 ? g : group_base(g & 1, t) + g / 2; }      // lane g's entry in step t's argument arrays
    Part part(const mihevc_session *s, int grp, int t) const
    {
        Part p;
        p.grp = grp; p.st = grp ? s->st_pre : s->st_compute;
        if (t == 0) { p.n = gl.batch[0]; for (int g = 0; g < p.n; g++) p.lanes.push_back(g); return p; }
        p.base = group_base(grp, t); p.n = group_size(grp, t);
        for (int k = 0; k < p.n; k++) p.lanes.push_back(groups == 1 ? k : 2 * k + grp);
        return p;
    }
    Chunk(const mihevc_session *s, int n_, GopLayout gl_)
        : n(n_), gops((int)gl_.glen.size()), steps(gl_.glen[0]), ring(s->ring), first_index(s->frames_in - n_), gl(std::move(gl_)), sl(s->w, s->h), lay(gops),
          flat_off((size_t)(steps + 1) * lay.total) {}
    // ring slot of step t; lane g's step t: GOP structure, output (display) index of its picture (cfg.bframes: steps are in decoding order)
    int slot_of(int t) const { return t == 0 ? 0 : 1 + (t - 1) % (ring - 1); }
    GopStep step(int g, int t) const { return gop_step(bf, t, gl.glen[(size_t)g]); }
    size_t fidx(int g, int t) const { return (size_t)(first_index + gl.gstart[(size_t)g] + step(g, t).pos); }
};

// GOP layout of the chunk (csrc/gop_plan.h).  Here: whether the scene-cut detector applies, and its one device call.  A session that codes one slice of
// the picture sees only its band, and the slices of a picture must agree on its type: no cut detection there.
template <typename T> int gop_layout(mihevc_session *s, int n, GopLayout &gl)
{
    std::vector<unsigned long long> diff;
    if (s->cfg.scenecut && s->cfg.slice_count <= 1 && n > 1 && s->cfg.min_keyint < s->keyint) {
        diff.assign((size_t)n, 0);
        if (int e = scene_differences<T>(s, n, diff)) return e;
    }
    const double per = (double)((s->w + 3) / 4) * ((s->h + 3) / 4) * (1 << (s->cfg.bit_depth - 8));
    gl = gop_plan(diff, per, n, s->keyint, s->cfg.min_keyint, s->cfg.gop_balance != 0, s->flushing, MAX_LANES, s->gop);
    return 0;
}

// slices that exchange rows: what the neighbours need to know about this band's buffers, then everybody's (csrc/slice_group.h)
int setup_halo(mihevc_session *s, int gops, int steps, Halo &h)
{
    if (!s->group) return 0;
    h.on = true;
    h.up = s->band > 0 ? 1 : 0; h.dn = s->band + 1 < s->n_bands ? 1 : 0;
    for (int dir = -1; dir <= 1; dir += 2) {      // bands whose rows lie within PAD_Y rows above / below this band, nearest first, with the rows each contributes
        int left = PAD_Y;
        for (int b = s->band + dir; b >= 0 && b < s->n_bands && left > 0; b += dir) {
            const int rows = std::min(left, s->band_h[b]);
            (dir < 0 ? h.reach_up : h.reach_dn).push_back({b, rows});
            (dir < 0 ? h.top : h.bottom) += rows;
            left -= rows;
        }
    }
    h.reach = (int)(h.reach_up.size() + h.reach_dn.size());
    h.jl = JobLayout(gops, h.reach);
    if (gops > kHaloLanes) { std::lock_guard<std::mutex> l(s->m); s->err = "too many GOP lanes for sliced pictures"; return MIHEVC_EINVAL; }
    BandPub &me = s->group->pub(s->band);
    me.device = s->device; me.w = s->w; me.h = s->h; me.is16 = s->is16;
    for (int g = 0; g < gops; g++)
        for (int k = 0; k < 2; k++)
            for (int i = 0; i < 3; i++) me.rec_p[g][k][i] = s->lane[g].rec_p[k][i];
    for (int i = 0; i < 3; i++) me.rec_stride[i] = s->lane[0].rec_stride[i];
    for (int k = 0; k < 2; k++) { me.x1_export[k] = s->x1_export[k]; me.ev_x1[k] = s->ev_x1[k]; me.ev_x2[k] = s->ev_x2[k]; }
    me.x1_lane_bytes = s->x1_lane_bytes;
    if (!s->group->barrier()) return fail(s, kPeerFailed);
    for (auto &v : {h.reach_up, h.reach_dn})
        for (auto &br : v) {
            const int dev = s->group->pub(br.first).device;
            if (dev == s->device || std::find(s->peers_enabled.begin(), s->peers_enabled.end(), dev) != s->peers_enabled.end()) continue;
            hipError_t e = hipDeviceEnablePeerAccess(dev, 0);
            (void)hipGetLastError();
            if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) return fail(s, std::string("hipDeviceEnablePeerAccess: ") + hipGetErrorString(e));
            s->peers_enabled.push_back(dev);
        }
    const size_t jneed = (size_t)steps * h.jl.total;
    if (int e = grow(s, s->jobs, jneed, 0xffff, true)) return e;
    h.hj = s->jobs.h; h.dj = (uint8_t *)s->jobs.d;
    memset(h.hj, 0, jneed);
    return 0;
}

// the neighbours' announcement `which` (1: X1 rows exported, 2: final pictures written) of group step G, then their event on the compute stream
int wait_neighbours(mihevc_session *s, const Halo &h, int which, long long G)
{
    for (auto *v : {&h.reach_up, &h.reach_dn})
        for (auto &br : *v) {
            if (!s->group->wait_for(br.first, which, G)) return fail(s, kPeerFailed);
            const BandPub &nb = s->group->pub(br.first);
            HIPCK(s, hipStreamWaitEvent(s->st_compute, (which == 1 ? nb.ev_x1 : nb.ev_x2)[G & 1], 0));
        }
    return 0;
}

CostParams prm_for(const mihevc_session *s, int qp)
{
    mihevc_cost_params c;
    mihevc_cost_params_for_qp(qp, s->cfg.bit_depth, s->me_range, &c);
    return CostParams{c.qp, c.qp_c, c.bit_depth, c.lambda_sad_q4, c.lambda_q4, c.me_range, s->tiles.cols, s->tiles.rows, s->cfg.intra_nxn != 0, s->cfg.intra_in_p != 0, s->cfg.pre_search != 0, s->cfg.rdo_zero != 0, s->cfg.chroma_modes != 0,
                      s->cfg.slice_count > 1 && !s->cfg.slice_halo && s->cfg.slice_index > 0, s->cfg.slice_count > 1 && !s->cfg.slice_halo && s->cfg.slice_index < s->cfg.slice_count - 1, std::max(0, s->cfg.rdo_cg), s->cfg.sign_hide};
}

// the chunk's argument blocks and, with cfg.pre_search, its 1/4-size source pictures and search centres: [n_pre pictures of (w/4)(h/4) bytes | n_pre x n_ctu x 2 int16]
template <typename T> int alloc_chunk(mihevc_session *s, Chunk<T> &c)
{
    c.n_pre = c.bf ? 2 * c.n : c.n;
    c.need = c.flat_off + (size_t)c.n_pre * sizeof(PreArgs<T>);
    if (int e = grow(s, s->args, c.need, 0xffff, true)) return e;      // whole 64 KiB: the next session's chunk finds the block in the cache
    c.ha = s->args.h; c.da = (uint8_t *)s->args.d;
    c.low_pic = (size_t)(s->w >> 2) * (s->h >> 2);
    const size_t low_bytes = ((size_t)c.n_pre * c.low_pic + 255) & ~(size_t)255;
    if (s->cfg.pre_search)
        if (int e = grow(s, s->low, low_bytes + (size_t)c.n_pre * s->n_ctu * 2 * sizeof(int16_t), 0xfffff, false)) return e;
    c.low = (uint8_t *)s->low.d;
    c.cen = (int16_t *)((uint8_t *)s->low.d + low_bytes);
    return 0;
}

// the row copies of lane g at step t: export (this band's first / last rows), import (the neighbours' rows next to it), pull (the neighbours' final
// pictures into the border rows of this band's reference)
template <typename T> void row_jobs(mihevc_session *s, const Chunk<T> &c, int t, int g, int prev, uint8_t *sym)
{
    const Halo &h = c.halo;
    mihevc_session::Lane &L = s->lane[g];
    const int w8 = s->w >> 3;
    const long long G = s->gstep + t;
    const size_t es = sizeof(T), part = s->x1_part_bytes;
    uint8_t *hj = h.hj + (size_t)t * h.jl.total;
    RowCopy *je = (RowCopy *)(hj + h.jl.exp) + (size_t)g * 8, *ji = (RowCopy *)(hj + h.jl.imp) + (size_t)g * 8;
    RowCopy *jp = (RowCopy *)(hj + h.jl.pull) + (size_t)g * 3 * std::max(1, h.reach);
    uint8_t *xe = (uint8_t *)s->x1_export[G & 1] + (size_t)g * s->x1_lane_bytes;
    const size_t off_pl[3] = {0, (size_t)kSeamRows * s->w * es, (size_t)kSeamRows * s->w * es + (size_t)(kSeamRows / 2) * (s->w / 2) * es};
    const size_t off_cu = off_pl[2] + (size_t)(kSeamRows / 2) * (s->w / 2) * es;
    mihevc_cu_rec *cu0 = (mihevc_cu_rec *)(sym + c.sl.cu);
    for (int side = 0; side < 2; side++) {          // export: this band's first / last rows -> [top part | bottom part]
        for (int i = 0; i < 3; i++) {
            const int pw = i ? s->w / 2 : s->w, ph = i ? s->h / 2 : s->h, rows = i ? kSeamRows / 2 : kSeamRows;
            je[side * 4 + i] = RowCopy{(const uint8_t *)L.work_p[i] + (size_t)(side ? ph - rows : 0) * L.work_stride[i] * es, xe + side * part + off_pl[i], (int)(pw * es), rows,
                                       (int)(L.work_stride[i] * es), (int)(pw * es)};
        }
        je[side * 4 + 3] = RowCopy{cu0 + (size_t)(side ? (s->h >> 3) - 1 : 0) * w8, xe + side * part + off_cu, (int)(w8 * sizeof(mihevc_cu_rec)), 1, 0, 0};
    }
    for (int side = 0; side < 2; side++) {          // import: the upper neighbour's bottom part -> the rows above this band; the lower neighbour's top part -> below
        if (!(side ? h.dn : h.up)) continue;
        const BandPub &nb = s->group->pub(s->band + (side ? 1 : -1));
        const uint8_t *xs = (const uint8_t *)nb.x1_export[G & 1] + (size_t)g * nb.x1_lane_bytes + (side ? 0 : part);
        for (int i = 0; i < 3; i++) {
            const int pw = i ? s->w / 2 : s->w, ph = i ? s->h / 2 : s->h, rows = i ? kSeamRows / 2 : kSeamRows;
            ji[side * 4 + i] = RowCopy{xs + off_pl[i], (uint8_t *)L.work_p[i] + ((ptrdiff_t)(side ? ph : -rows) * L.work_stride[i]) * (ptrdiff_t)es, (int)(pw * es), rows,
                                       (int)(pw * es), (int)(L.work_stride[i] * es)};
        }
        ji[side * 4 + 3] = RowCopy{xs + off_cu, side ? cu0 + (size_t)(s->h >> 3) * w8 : cu0 - w8, (int)(w8 * sizeof(mihevc_cu_rec)), 1, 0, 0};
    }
    if (t == 0) return;
    int k = 0;                                      // pull: the final reconstruction either side of the seams -> the border rows of this band's reference
    for (int side = 0; side < 2; side++) {
        int done = 0;
        for (auto &br : side ? h.reach_dn : h.reach_up) {
            const BandPub &nb = s->group->pub(br.first);
            for (int i = 0; i < 3; i++) {
                const int pw = i ? s->w / 2 : s->w, ph = i ? s->h / 2 : s->h, nh = i ? nb.h / 2 : nb.h, rows = i ? br.second / 2 : br.second, dn_ = i ? done / 2 : done;
                const uint8_t *src = (const uint8_t *)nb.rec_p[g][prev][i] + (size_t)(side ? 0 : nh - rows) * nb.rec_stride[i] * es;
                uint8_t *dst = (uint8_t *)L.rec_p[prev][i] + ((ptrdiff_t)(side ? ph + dn_ : -(dn_ + rows)) * L.rec_stride[i]) * (ptrdiff_t)es;
                jp[k++] = RowCopy{src, dst, (int)(pw * es), rows, (int)(nb.rec_stride[i] * es), (int)(L.rec_stride[i] * es)};
            }
            done += br.second;
        }
    }
}

// the argument blocks of lane g at step t (host staging; the chunk uploads them once), its pre-search blocks, its row copies
template <typename T> void build_step_args(mihevc_session *s, const Chunk<T> &c, int t, int g)
{
    const SymLayout &sl = c.sl;
    const Halo &h = c.halo;
    const GopStep gs = c.step(g, t);
    const int fi = c.gl.gstart[(size_t)g] + gs.pos;
    mihevc_session::Lane &L = s->lane[g];
    Src &src = s->pending[fi];
    StepView<T> hv(c.ha, c.lay, t);
    const int a = c.at(t, g);
    struct { IntraArgs<T> &intra; InterArgs<T> &inter; DeblockArgs<T> &dbk_v, &dbk_h; SaoArgs<T> &sao; } A{hv.intra[a], hv.inter[a], hv.dbk_v[a], hv.dbk_h[a], hv.sao[a]};
    uint8_t *sym = L.sym_dev[c.slot_of(t)];
    const CostParams P = prm_for(s, t == 0 ? s->qp_i : s->qp_p);      // provisional; the controller patches it per step
    for (int i = 0; i < 3; i++) {
        A.intra.src[i] = mkc<T>(src.p[i], src.stride[i]); A.intra.rec[i] = mk<T>(L.work_p[i], L.work_stride[i]);
        A.inter.src[i] = mkc<T>(src.p[i], src.stride[i]); A.inter.ref[i] = mkc<T>(L.rec_p[gs.prev][i], L.rec_stride[i]);
        A.inter.rec[i] = mk<T>(L.work_p[i], L.work_stride[i]);
        A.dbk_v.rec[i] = A.dbk_h.rec[i] = mk<T>(L.work_p[i], L.work_stride[i]);
        A.sao.src[i] = mkc<T>(src.p[i], src.stride[i]); A.sao.dbk[i] = mkc<T>(L.work_p[i], L.work_stride[i]);
        A.sao.out[i] = mk<T>(L.rec_p[gs.cur][i], L.rec_stride[i]);
    }
    A.intra.w = A.inter.w = A.dbk_v.w = A.dbk_h.w = A.sao.w = s->w;
    A.intra.h = A.inter.h = A.dbk_v.h = A.dbk_h.h = A.sao.h = s->h;
    A.intra.ctus_w = A.inter.ctus_w = A.sao.ctus_w = s->ctus_w; A.intra.ctus_h = s->ctus_h;
    A.intra.prm = A.inter.prm = A.sao.prm = P;
    A.intra.cu = A.inter.cu = (mihevc_cu_rec *)(sym + sl.cu);
    A.dbk_v.cu = A.dbk_h.cu = (const mihevc_cu_rec *)(sym + sl.cu);
    A.sao.halo_top = h.top; A.sao.halo_bottom = h.bottom;
    // SAO on: the CTU programs of the SAO kernel deblock their own tile first (one launch for 8.7.2 + 8.7.3, the work picture stays as the analysis left it)
    A.sao.cu = s->cfg.sao ? (const mihevc_cu_rec *)(sym + sl.cu) : nullptr;
    if (h.on) {
        // deblocking runs over the band EXTENDED by the rows the neighbours hand over (kSeamRows of their pre-deblock reconstruction + one row of CU
        // records either side): the seams are inner edges of that picture
        for (int i = 0; i < 3; i++) {
            const int tr = h.up ? (i ? kSeamRows / 2 : kSeamRows) : 0;
            A.dbk_v.rec[i] = A.dbk_h.rec[i] = mk<T>((T *)L.work_p[i] - (ptrdiff_t)tr * L.work_stride[i], L.work_stride[i]);
        }
        A.dbk_v.h = A.dbk_h.h = s->h + kSeamRows * (h.up + h.dn);
        A.dbk_v.cu = A.dbk_h.cu = (const mihevc_cu_rec *)(sym + sl.cu) - (h.up ? s->w >> 3 : 0);
        row_jobs<T>(s, c, t, g, gs.prev, sym);
    }
    // levels go straight to the pinned host block (device-mapped): only TUs with a non-zero level are stored, so the
    // 6 MB/picture coefficient planes never cross PCIe as a blit (profiles/r01: copyBuffer was 17 % of GPU time)
    uint8_t *symh = L.sym_host[c.slot_of(t)];
    int16_t *c3[3] = {(int16_t *)(symh + sl.cy), (int16_t *)(symh + sl.cu_), (int16_t *)(symh + sl.cv)};
    for (int i = 0; i < 3; i++) A.intra.coef[i] = A.inter.coef[i] = c3[i];
    A.intra.sparse_coef = A.inter.sparse_coef = 1;
    A.intra.diagonal = 0;
    A.inter.centers = nullptr; A.inter.me = L.me;
    for (int i = 0; i < 3; i++) A.inter.ref1[i] = gs.type == 0 ? mkc<T>(L.rec_p[gs.nxt][i], L.rec_stride[i]) : Plane<const T>{nullptr, 0};
    A.inter.centers1 = nullptr; A.inter.me1 = gs.type == 0 ? L.me1 : nullptr;
    if (s->cfg.pre_search) {       // search centres: the chunk's pre-search fills them for every picture (encode_chunk)
        const size_t idx = (size_t)fi, ridx = (size_t)(c.gl.gstart[(size_t)g] + std::max(0, gs.ref_pos));
        PreArgs<T> &P4 = ((PreArgs<T> *)(c.ha + c.flat_off))[idx];
        P4.src = A.inter.src[0]; P4.ref = A.inter.src[0];
        P4.lsrc = c.low + idx * c.low_pic; P4.lref = c.low + (t > 0 ? ridx : idx) * c.low_pic;      // against the SOURCE of the picture it will predict from; an IDR picture's centres are never read
        P4.w = s->w; P4.h = s->h; P4.bit_depth = s->cfg.bit_depth; P4.centers = c.cen + idx * (size_t)s->n_ctu * 2; P4.cost = nullptr;
        if (t > 0) A.inter.centers = P4.centers;
        if (c.bf) {                // the second block: a B picture against the source of the anchor AFTER it (other pictures: a copy of the first, never read)
            PreArgs<T> &P5 = ((PreArgs<T> *)(c.ha + c.flat_off))[(size_t)c.n + idx];
            P5 = P4;
            P5.lsrc = c.low + ((size_t)c.n + idx) * c.low_pic; P5.centers = c.cen + ((size_t)c.n + idx) * (size_t)s->n_ctu * 2;
            if (gs.type == 0) { P5.lref = c.low + (idx + 1) * c.low_pic; A.inter.centers1 = P5.centers; }
        }
    }
    // P pictures: the inter pass leaves per-CTU costs for the intra second pass, which runs on the same work picture,
    // records and levels with the one-tile PPS 0 geometry
    const bool ipass = gs.type == 1 && s->cfg.intra_in_p;
    A.inter.ip = ipass ? L.ip : nullptr;
    A.intra.ip = ipass ? L.ip : nullptr;
    A.intra.plan = t == 0 ? L.plan : nullptr;      // P pictures' second pass plans and codes a CTU inside one workgroup
    if (t > 0) { A.intra.prm.tile_cols = s->ptiles.cols; A.intra.prm.tile_rows = s->ptiles.rows; }
    A.dbk_v.bit_depth = A.dbk_h.bit_depth = s->cfg.bit_depth; A.dbk_v.dir = 0; A.dbk_h.dir = 1;
    A.dbk_v.y_org = A.dbk_h.y_org = h.up ? kSeamRows : 0;
    A.sao.sao = s->cfg.sao ? (mihevc_sao_ctu *)(sym + sl.sao) : nullptr;
    A.sao.sse = (unsigned long long *)(sym + sl.sse);
    A.sao.sse_ctu = s->cfg.sao ? (uint32_t *)(sym + sl.sse_ctu) : nullptr;
    A.intra.est = A.inter.est = (unsigned long long *)(sym + sl.est);
}

// the QP of lane g's picture at step t into its argument blocks and frame record
template <typename T> void patch_qp(mihevc_session *s, const Chunk<T> &c, int t, int g, int qp)
{
    StepView<T> hv(c.ha, c.lay, t);
    const int a = c.at(t, g);
    hv.intra[a].prm = hv.inter[a].prm = hv.sao[a].prm = prm_for(s, qp);
    if (t > 0) { hv.intra[a].prm.tile_cols = s->ptiles.cols; hv.intra[a].prm.tile_rows = s->ptiles.rows; }
    std::lock_guard<std::mutex> l(s->m);
    auto &fr = s->frames[c.fidx(g, t)];
    fr.qp = qp; fr.type = type_of_step(c.bf, t);
}

// lane g's frame records of steps [0, upto), for the rate controller
template <typename T> std::vector<FrameRec> lane_records(mihevc_session *s, const Chunk<T> &c, int g, int upto)
{
    std::vector<FrameRec> v((size_t)upto);
    std::lock_guard<std::mutex> l(s->m);
    for (int j = 0; j < upto; j++) v[(size_t)j] = s->frames[c.fidx(g, j)];
    return v;
}

// slices with one rate plan: the CABAC sizes (with_est: and the estimates) of the pictures `idx`, summed over the slices of the picture
int slice_sums(mihevc_session *s, const std::vector<size_t> &idx, bool with_est)
{
    const size_t n = idx.size();
    std::vector<double> v(with_est ? 2 * n : n);
    {
        std::lock_guard<std::mutex> l(s->m);
        for (size_t i = 0; i < n; i++) { v[i] = (double)s->frames[idx[i]].bits_local; if (with_est) v[n + i] = (double)s->frames[idx[i]].est_local; }
    }
    if (int e = group_sum(s, v)) return e;
    std::lock_guard<std::mutex> l(s->m);
    for (size_t i = 0; i < n; i++) { auto &fr = s->frames[idx[i]]; fr.bits = (long long)v[i]; if (with_est) { fr.est_q4 = (unsigned long long)v[n + i]; fr.est_known = true; } }
    return 0;
}

// The rate estimates the analyses of `lanes` leave in ring slot `slot` (device symbol blocks), in two halves.  queue_estimates goes right behind the launches
// that produce them: one 8-byte copy per lane on the compute stream into the session's pinned words.  wait_estimates is the ONE wait of the host for the
// compute stream (a blocking copy per lane was a round trip per lane, behind a synchronise of its own), then the words, summed over the slices of the picture
int queue_estimates(mihevc_session *s, const SymLayout &sl, int slot, const std::vector<int> &lanes)
{
    if (!s->est_host) HIPCK(s, s->est_host.alloc(s->device, MAX_LANES * sizeof(unsigned long long), true));
    for (size_t k = 0; k < lanes.size(); k++)
        HIPCK(s, hipMemcpyAsync(s->est_host + k, s->lane[lanes[k]].sym_dev[slot] + sl.est, sizeof(unsigned long long), hipMemcpyDeviceToHost, s->st_compute));
    return 0;
}
int wait_estimates(mihevc_session *s, size_t n, std::vector<unsigned long long> &out)
{
    HIPCK(s, hipStreamSynchronize(s->st_compute));
    std::vector<double> v(n, 0.0);
    for (size_t k = 0; k < n; k++) v[k] = (double)s->est_host[k];
    if (int e = group_sum(s, v)) return e;
    out.assign(v.begin(), v.end());
    return 0;
}
std::vector<int> first_lanes(int n) { std::vector<int> v((size_t)n); std::iota(v.begin(), v.end(), 0); return v; }

int mark(mihevc_session *s, hipStream_t st, int stage, int pictures, bool begin)       // bracket a stage with events when profiling, on the stream its launch goes to
{
    if (!s->cfg.profile_stages || (s->cfg.profile_stages == 2 && stage != 2)) return 0;      // 2: the dominant stage (inter_ctu) only
    size_t need_ev = s->marks.size() * 2 + 2;
    while (s->ev_pool.size() < need_ev) { s->ev_pool.emplace_back(hipEventDefault); if (!s->ev_pool.back()) return fail(s, "hipEventCreate failed"); }
    if (begin) { s->marks.push_back({stage, pictures, s->marks.size() * 2}); HIPCK(s, hipEventRecord(s->ev_pool[s->marks.back().ev], st)); }
    else HIPCK(s, hipEventRecord(s->ev_pool[s->marks.back().ev + 1], st));
    return 0;
}
#define STAGE(st, idx, pics, call) do { if (int e_ = mark(s, st, idx, pics, true)) return e_; HIPCK(s, call); if (int e_ = mark(s, st, idx, pics, false)) return e_; } while (0)

// rate feedback in front of step t (rate control only).  Slices with one rate plan: the CABAC sizes of step t - p_slots, summed over the slices.  Then, with
// a fixed lag of two steps, the estimates of step t - 2: wait for its symbol copy (step t - 1 is already queued behind it, so the device never idles).  A fixed
// lag makes the QP sequence reproducible.
template <typename T> int rate_feedback(mihevc_session *s, const Chunk<T> &c, const Part &p, int t)
{
    const int p_slots = s->ring - 1;
    if (c.halo.on && s->rc.rc_on && t - p_slots >= 1) {
        // the pictures of step t - p_slots have left the CABAC jobs of EVERY slice once all slices are here
        std::vector<size_t> idx;
        for (int g = 0; g < c.gl.batch[(size_t)(t - p_slots)]; g++) idx.push_back(c.fidx(g, t - p_slots));
        if (int e = slice_sums(s, idx, false)) return e;
    }
    // the copy-stream work of this group's step t - 2 (SSE, hash, SSIM) still reads the picture buffers this step reuses (step 0: all lanes, group 0's slot 0)
    if (t >= 2) HIPCK(s, hipStreamWaitEvent(p.st, s->slot[t == 2 ? 0 : p.grp][c.slot_of(t - 2)].copy, 0));
    if (!s->rc.rc_on || t < 3) return 0;
    const int j = t - 2;
    const Part pj = c.part(s, p.grp, j);      // this group's lanes at step j (a superset of its lanes now)
    HIPCK(s, hipEventSynchronize(s->slot[p.grp][c.slot_of(j)].copy));
    std::vector<double> v((size_t)pj.n);
    for (int k = 0; k < pj.n; k++) v[(size_t)k] = (double)*(const unsigned long long *)(s->lane[pj.lanes[(size_t)k]].sym_host[c.slot_of(j)] + c.sl.est);
    if (int e = group_sum(s, v)) return e;
    std::lock_guard<std::mutex> l(s->m);
    for (int k = 0; k < pj.n; k++) { auto &fr = s->frames[c.fidx(pj.lanes[(size_t)k], j)]; if (!fr.est_known) { fr.est_q4 = (unsigned long long)v[(size_t)k]; fr.est_known = true; } }
    return 0;
}

// First chunk of a session: rho is only a prior (1/16).  Measure it: analyse every GOP's first P picture once against the UNFILTERED reconstruction of
// the IDR analysis (copied + padded into the reference buffer the real step 0 overwrites afterwards) at the wanted IDR QP + 3, and read the estimate.
// Costs one P step per session.  The trial runs in the block behind the chunk's last step.
// Its first half is everything that does not depend on the wanted QPs: it runs while the device is still busy with the IDR analyses whose estimates decide them
template <typename T> int rho_trial_prepare(mihevc_session *s, const Chunk<T> &c)
{
    const int B1 = c.gl.batch[1], tb = c.steps;
    memcpy(c.ha + (size_t)tb * c.lay.total, c.ha + (size_t)1 * c.lay.total, c.lay.total);
    StepView<T> tv(c.ha, c.lay, tb), h0(c.ha, c.lay, 0), h1(c.ha, c.lay, 1);
    for (int g = 0; g < B1; g++) {
        mihevc_session::Lane &L = s->lane[g];
        const int a = c.at(1, g);      // the trial block is a copy of step 1's: its order
        tv.sao[a] = h0.sao[c.at(0, g)];
        tv.sao[a].sao = nullptr; tv.sao[a].sse = nullptr; tv.sao[a].sse_ctu = nullptr; tv.sao[a].cu = nullptr;
        tv.sao[a].halo_top = tv.sao[a].halo_bottom = 0;      // the trial predicts from this band's own unfiltered picture with a replicated border
        tv.inter[a] = h1.inter[a];
        for (int i = 0; i < 3; i++) tv.inter[a].rec[i] = mk<T>(L.rec_p[1][i], L.rec_stride[i]);
        tv.inter[a].ip = nullptr;
        HIPCK(s, hipMemsetAsync(L.sym_dev[c.slot_of(1)] + c.sl.sse, 0, 4 * sizeof(unsigned long long), s->st_compute));
    }
    return 0;
}
// the second half: the trial QPs into the prepared block, the launches, one wait for the estimates
template <typename T> int rho_trial(mihevc_session *s, const Chunk<T> &c, const std::vector<int> &want, const std::vector<unsigned long long> &ev, const std::vector<int> &qa)
{
    const int B1 = c.gl.batch[1], tb = c.steps;
    StepView<T> tv(c.ha, c.lay, tb), dtv(c.da, c.lay, tb);
    std::vector<int> qp_trial((size_t)B1);
    for (int g = 0; g < B1; g++) {
        qp_trial[(size_t)g] = RateControl::trial_qp(want[(size_t)g]);
        tv.inter[c.at(1, g)].prm = prm_for(s, qp_trial[(size_t)g]);
    }
    HIPCK(s, hipMemcpyAsync(c.da + (size_t)tb * c.lay.total, c.ha + (size_t)tb * c.lay.total, c.lay.total, hipMemcpyHostToDevice, s->st_compute));
    HIPCK(s, launch_sao<T>(s->st_compute, dtv.sao, s->w, s->h, B1, false));
    HIPCK(s, launch_pad<T>(s->st_compute, dtv.sao, s->w, s->h, B1));
    if (s->cfg.pre_search) HIPCK(s, hipStreamWaitEvent(s->st_compute, s->ev_pre, 0));      // the chunk's search centres
    HIPCK(s, launch_me_search<T>(s->st_compute, dtv.inter, s->n_ctu, B1, s->me_range));
    HIPCK(s, launch_inter_ctu<T>(s->st_compute, dtv.inter, s->n_ctu, B1, s->me_range));
    if (int e = queue_estimates(s, c.sl, c.slot_of(1), first_lanes(B1))) return e;
    std::vector<unsigned long long> ep;
    if (int e = wait_estimates(s, (size_t)B1, ep)) return e;
    s->rc.measure_rho(ep, qp_trial, ev, qa);
    return 0;
}

// step 0: the IDR picture of every lane, the chunk's pre-search beside it, and under rate control the IDR QP decision (csrc/ratectl.h): one analysis,
// the rho trial in a session's first chunk, a second analysis of the lanes whose wanted QP is far from the first one's
template <typename T> int idr_step(mihevc_session *s, const Chunk<T> &c, std::vector<int> &qp_step)
{
    const int B = c.gl.batch[0];
    StepView<T> dv(c.da, c.lay, 0), hv(c.ha, c.lay, 0);
    HIPCK(s, hipMemcpyAsync(c.da, c.ha, c.lay.total, hipMemcpyHostToDevice, s->st_compute));
    for (int g = 0; g < B; g++) HIPCK(s, hipMemsetAsync(s->lane[g].sym_dev[0] + c.sl.sse, 0, 4 * sizeof(unsigned long long), s->st_compute));
    STAGE(s->st_compute, 0, B, launch_intra_picture<T>(s->st_compute, dv.intra, s->ctus_w, s->ctus_h, B, s->tiles.cols, s->tiles.rows, s->cfg.pre_search ? s->ev_args : nullptr));
    if (s->rc.rc_on) { if (int e = queue_estimates(s, c.sl, 0, first_lanes(B))) return e; }
    // cfg.pre_search: the search centres of EVERY picture of the chunk come from the 1/4-size SOURCE pictures (this picture against the one before it: nothing
    // in it waits for a reconstruction), in two launches on a stream of their own: the work (7 % of a clip's device time when it ran inside every step) sits
    // beside the anti-diagonal chain, which leaves most of the device idle, not beside k_intra_plan (both want the ALUs).  The first P step waits for ev_pre.
    if (s->cfg.pre_search) {
        HIPCK(s, hipStreamWaitEvent(s->st_pre, s->ev_args, 0));
        HIPCK(s, launch_pre_search_chunk<T>(s->st_pre, (const PreArgs<T> *)(c.da + c.flat_off), s->w, s->h, s->n_ctu, c.n_pre));
        HIPCK(s, hipEventRecord(s->ev_pre, s->st_pre));
    }
    if (!s->rc.rc_on) return 0;
    // the host's part of step 0 that needs no estimate runs beside the analyses; the device stands still from the wait below until the next launch
    const bool trial = !s->rc.rho_measured && c.steps > 1 && c.gl.batch[1] > 0;
    if (trial) { if (int e = rho_trial_prepare<T>(s, c)) return e; }
    std::vector<unsigned long long> ev, e2;
    if (int e = wait_estimates(s, (size_t)B, ev)) return e;
    const std::vector<int> qa(qp_step);                       // QP each lane's current analysis was made at
    std::vector<int> want((size_t)B);
    for (int g = 0; g < B; g++) want[(size_t)g] = s->rc.want_idr(g, ev[(size_t)g], qa[(size_t)g]);
    if (trial) {
        if (int e = rho_trial<T>(s, c, want, ev, qa)) return e;
        for (int g = 0; g < B; g++) want[(size_t)g] = s->rc.want_idr(g, ev[(size_t)g], qa[(size_t)g]);
    }
    std::vector<int> redo;
    for (int g = 0; g < B; g++)
        if (RateControl::redo_idr(want[(size_t)g], qa[(size_t)g])) redo.push_back(g);
    if (!redo.empty()) {
        // second analysis of those lanes at the wanted QP into the same buffers (every CTU, record and non-zero TU is rewritten;
        // levels of TUs that are zero now are never read by the entropy coder): argument blocks compacted behind the first B
        for (size_t k = 0; k < redo.size(); k++) {
            const int g = redo[k];
            qp_step[(size_t)g] = want[(size_t)g];
            patch_qp<T>(s, c, 0, g, qp_step[(size_t)g]);
            hv.intra[B + (int)k] = hv.intra[c.at(0, g)];
            HIPCK(s, hipMemsetAsync(s->lane[g].sym_dev[0] + c.sl.sse, 0, 4 * sizeof(unsigned long long), s->st_compute));
        }
        HIPCK(s, hipMemcpyAsync(c.da, c.ha, c.lay.total, hipMemcpyHostToDevice, s->st_compute));
        STAGE(s->st_compute, 0, (int)redo.size(), launch_intra_picture<T>(s->st_compute, dv.intra + B, s->ctus_w, s->ctus_h, (int)redo.size(), s->tiles.cols, s->tiles.rows, nullptr));
        if (int e = queue_estimates(s, c.sl, 0, redo)) return e;
        if (int e = wait_estimates(s, redo.size(), e2)) return e;
        for (size_t k = 0; k < redo.size(); k++) ev[(size_t)redo[k]] = e2[k];
    }
    s->rc.idr_settled(qp_step);
    std::lock_guard<std::mutex> l(s->m);
    for (int g = 0; g < B; g++) { auto &fr = s->frames[c.fidx(g, 0)]; fr.est_q4 = ev[(size_t)g]; fr.est_known = true; }
    return 0;
}

// a P or B step: head, integer search, inter CTU programs (+ the intra second pass of P pictures)
template <typename T> int inter_step(mihevc_session *s, const Chunk<T> &c, const Part &p, int t)
{
    const int B = p.n;
    hipStream_t st = p.st;
    // this part's entries of the step's arrays, and of the previous step's (the same lanes in the same order: a group's lanes only ever drop off its end)
    StepView<T> dv(c.da, c.lay, t, p.base), hv(c.ha, c.lay, t, p.base), pv(c.da, c.lay, t - 1, c.group_base(p.grp, t - 1));
    // the step's QPs reach the device inside one tiny launch that also zeroes the slot's SSE + estimate accumulators; everything
    // else in the step's argument block went up with the chunk
    // The same launch pads the border of the previous step's pictures (nothing before this step's searches reads it) and makes the 1/4-size
    // pictures: one launch boundary on the compute stream instead of three (~6 us each, profiles/r02_e: kernel time 733 of 797 us per step).
    StepParams sp{};
    sp.p_tile_cols = s->ptiles.cols; sp.p_tile_rows = s->ptiles.rows;
    for (int g = 0; g < B; g++) sp.prm[g] = hv.inter[g].prm;
    if (c.halo.on && c.halo.reach > 0) {
        // X2: the final reconstruction either side of the seams, straight out of the neighbours' pictures of the previous step, into the border
        // rows of this band's reference pictures (the pad below fills in their left / right ends and whatever lies beyond the whole picture)
        if (int e = wait_neighbours(s, c.halo, 2, s->gstep + t - 1)) return e;
        HIPCK(s, launch_copy_rows(st, c.halo.jobs(t, c.halo.jl.pull), B * 3 * c.halo.reach, 16));
    }
    HIPCK(s, launch_prep_p_step<T>(st, pv.sao, (const PreArgs<T> *)nullptr, dv.intra, dv.inter, dv.sao, sp, s->w, s->h, B));
    if (t == 1 && s->cfg.pre_search) HIPCK(s, hipStreamWaitEvent(st, s->ev_pre, 0));      // the chunk's search centres (st_pre, under the IDR step)
    // stage 1 = the integer search around the chunk's search centres (a B picture: against both anchors)
    const bool bstep = type_of_step(c.bf, t) == 0;
    if (int e_ = mark(s, st, 1, B, true)) return e_;
    HIPCK(s, launch_me_search<T>(st, dv.inter, s->n_ctu, B, s->me_range, 0));
    if (bstep) HIPCK(s, launch_me_search<T>(st, dv.inter, s->n_ctu, B, s->me_range, 1));
    if (int e_ = mark(s, st, 1, B, false)) return e_;
    if (bstep) STAGE(st, 2, B, launch_inter_ctu_b<T>(st, dv.inter, s->n_ctu, B, s->me_range));
    else STAGE(st, 2, B, launch_inter_ctu<T>(st, dv.inter, s->n_ctu, B, s->me_range));
    if (s->cfg.intra_in_p && !bstep) STAGE(st, 7, B, launch_intra_p<T>(st, dv.intra, s->n_ctu, B));
    return 0;
}

// the loop filter of step t (with the rows the neighbour slices hand over), then the step's symbols to the host on the copy stream
template <typename T> int filter_and_copy(mihevc_session *s, const Chunk<T> &c, const Part &p, int t)
{
    const int B = p.n, slot = c.slot_of(t);
    hipStream_t st = p.st;
    const Halo &h = c.halo;
    const SymLayout &sl = c.sl;
    const long long G = s->gstep + t;
    StepView<T> dv(c.da, c.lay, t, p.base);
    if (h.on) {
        // X1: kSeamRows rows of the pre-deblock reconstruction + one row of CU records either side of every seam.  Every band puts its own first and last
        // rows where its neighbours can read them (the band's picture is deblocked in place right after), then takes the neighbours'
        HIPCK(s, launch_copy_rows(st, h.jobs(t, h.jl.exp), B * 8, 8));
        HIPCK(s, hipEventRecord(s->ev_x1[G & 1], st));
        s->group->announce(s->band, 1, G);
        if (int e = wait_neighbours(s, h, 1, G)) return e;
        if (h.up + h.dn) HIPCK(s, launch_copy_rows(st, h.jobs(t, h.jl.imp), B * 8, 8));
    }
    if (!s->cfg.sao) STAGE(st, 3, B, launch_deblock<T>(st, dv.dbk_v, dv.dbk_h, s->w, s->h + (h.on ? kSeamRows * (h.up + h.dn) : 0), B));
    STAGE(st, 4, B, launch_sao<T>(st, dv.sao, s->w, s->h, B, s->cfg.sao != 0));
    if (h.on) {
        HIPCK(s, hipEventRecord(s->ev_x2[G & 1], st));
        s->group->announce(s->band, 2, G);
    }
    HIPCK(s, hipEventRecord(s->slot[p.grp][slot].compute, st));      // (the border pad of these pictures is part of the next step's first launch)
    HIPCK(s, hipStreamWaitEvent(s->st_copy, s->slot[p.grp][slot].compute, 0));
    // SSE (statistics only): the SAO programs left every CTU's squared error in the symbol block's device tail; one small launch on the copy stream, in
    // front of the symbol copies that carry its sums, adds them up.  (Until round 3 a pass of its own re-read source and reconstruction here: 7 MB per
    // picture and 25 us per step beside the compute stream.)  Without SAO that pass still runs: k_sao_apply is a plain copy and has no source.
    if (s->cfg.sao) HIPCK(s, launch_sse_fold<T>(s->st_copy, dv.sao, s->n_ctu, B));
    else HIPCK(s, launch_frame_sse<T>(s->st_copy, dv.sao, B));
    // decoded picture hash of the final pictures (coded area only: the border is the next step's pad), in front of the symbol copies that carry it.
    // The group's stream reuses these picture buffers two steps later, behind ev_copy of this step (rate_feedback).  The one copy stream takes both groups'
    // work in turn, which also keeps the shared hash_part / ssim_part scratch to one launch at a time
    if (s->cfg.pic_hash >= 2) HIPCK(s, launch_pic_hash<T>(s->st_copy, dv.sao, s->w, s->h, B, s->cfg.pic_hash - 1, s->hash_part, sl.hash - sl.sse));
    // SSIM of the same pictures against their sources.  The reconstructions are safe here as for the hash.  The sources: the chunk's source pictures are written by
    // nothing while the chunk runs (uploads of the NEXT chunk's frames go to other buffers: a chunk's buffers return to the free list only at its end, behind
    // hipStreamSynchronize(st_copy)), and planes borrowed from the caller (mihevc_send_frame_device) stay valid and unmodified until the picture's packet is out,
    // which is behind ev_copy of this step
    if (s->cfg.ssim) HIPCK(s, launch_ssim<T>(s->st_copy, dv.sao, s->w, s->h, B, s->ssim_part, sl.ssim - sl.sse));
    for (int k = 0; s->cfg.pic_hash == 1 && k < B; k++) {      // MD5: the picture to pinned memory for the CABAC job (no wait here)
        const int g = p.lanes[(size_t)k];
        uint8_t *dst = s->lane[g].md5_host[slot];
        const size_t es = esize(s);
        for (int i = 0; i < 3; i++) {
            const int pw = i ? s->w / 2 : s->w, ph = i ? s->h / 2 : s->h;
            HIPCK(s, hipMemcpy2DAsync(dst, pw * es, s->lane[g].rec_p[c.step(g, t).cur][i], s->lane[g].rec_stride[i] * es, pw * es, ph, hipMemcpyDeviceToHost, s->st_copy));
            dst += (size_t)pw * ph * es;
        }
    }
    for (int k = 0; k < B; k++) {   // CU records, then SAO parameters + SSE + rate estimate (the level planes were written to the host block directly)
        const int g = p.lanes[(size_t)k];
        uint8_t *hd = s->lane[g].sym_host[slot], *dd = s->lane[g].sym_dev[slot];
        HIPCK(s, hipMemcpyAsync(hd + sl.cu, dd + sl.cu, sl.cu_bytes, hipMemcpyDeviceToHost, s->st_copy));
        HIPCK(s, hipMemcpyAsync(hd + sl.sao, dd + sl.sao, sl.total - sl.sao, hipMemcpyDeviceToHost, s->st_copy));
    }
    for (int k = 0; s->keep_recon && k < B; k++) {
        const int g = p.lanes[(size_t)k];
        std::vector<uint16_t> &dst = s->recon[(int64_t)c.fidx(g, t)];
        const size_t es = esize(s);
        dst.assign((size_t)s->w * s->h * 3 / 2, 0);
        std::vector<uint8_t> tmp((size_t)s->w * s->h * 3 / 2 * es);
        size_t off = 0;
        HIPCK(s, hipStreamSynchronize(st));
        for (int i = 0; i < 3; i++) {
            int pw = i ? s->w / 2 : s->w, ph = i ? s->h / 2 : s->h;
            HIPCK(s, hipMemcpy2D(tmp.data() + off * es, pw * es, s->lane[g].rec_p[c.step(g, t).cur][i], s->lane[g].rec_stride[i] * es, pw * es, ph, hipMemcpyDeviceToHost));
            off += (size_t)pw * ph;
        }
        for (size_t i = 0; i < dst.size(); i++) dst[i] = s->is16 ? ((uint16_t *)tmp.data())[i] : tmp[i];
    }
    HIPCK(s, hipEventRecord(s->slot[p.grp][slot].copy, s->st_copy));
    return 0;
}
#undef STAGE

// CABAC of step t: one job per picture on the host pool, behind the step's symbol copy.  The pool's threads are shared by the pictures of the step
// (their tiles, when the picture has several: cfg.p_tiles / IDR grid)
template <typename T> void hand_out(mihevc_session *s, const Chunk<T> &c, const Part &p, int t, const std::vector<int> &qp_step)
{
    const int B = p.n, slot = c.slot_of(t);
    { std::lock_guard<std::mutex> l(s->m); s->slot[p.grp][slot].jobs_open += B; }
    // (the step's pictures, not the part's: what a picture's job is cut into, and with it the order its tiles are coded in, does not depend on the grouping)
    const int parts_wanted = std::max(1, s->host_threads / std::max(1, c.gl.batch[(size_t)t]));
    for (int k = 0; k < B; k++) {
        const int g = p.lanes[(size_t)k];
        const GopStep gs = c.step(g, t);
        const int gstart = c.gl.gstart[(size_t)g];
        PictureJob *j = new PictureJob();
        j->s = s; j->grp = p.grp; j->slot = slot; j->lane_i = g; j->index = (int64_t)c.fidx(g, t); j->pts = s->pending[gstart + gs.pos].pts;
        // packets leave in DECODING order: place t of the GOP; dts = the pts of the frame at that place in display order, one frame earlier when
        // B pictures reorder (an anchor is decoded one picture before the B picture in front of it is shown)
        j->dec_index = c.first_index + gstart + t;
        j->reorder = s->cfg.bframes != 0;
        j->dts = s->pending[gstart + t].pts - (j->reorder ? s->pts_step : 0);
        j->pic.ref_dist = gs.type == 1 ? gs.pos - gs.ref_pos : 0;
        j->dec_pos = t;
        j->prev_gop_len = c.gl.prev_len[(size_t)g];
        j->slice_type = gs.type; j->poc = gs.pos; j->qp = qp_step[(size_t)k]; j->first_of_stream = j->dec_index == 0;
        j->pic.slice_type = j->slice_type; j->pic.poc = gs.pos; j->pic.qp = j->qp;
        picture_symbols(s, j->slot, g, j->pic);
        j->n_tiles = picture_tiles(s->cfg, j->pic);
        j->parts = std::min(j->n_tiles, parts_wanted);
        j->sub.resize((size_t)j->n_tiles);
        const bool md5 = s->cfg.pic_hash == 1;
        j->left.store(j->parts + (md5 ? 1 : 0));
        hipEvent_t ev = s->slot[p.grp][slot].copy;
        for (int part = 0; part < j->parts; part++)
            s->pool->submit([s, j, part, ev] {
                (void)hipSetDevice(s->device);          // worker threads start on device 0: wait on the event in its own device's context
                (void)hipEventSynchronize(ev);
                entropy_part(j, part);
            });
        if (md5)
            s->pool->submit([s, j, ev] {
                (void)hipSetDevice(s->device);
                (void)hipEventSynchronize(ev);
                md5_part(j);
            });
    }
}

// behind the chunk's last step, every CABAC job done: slices with one rate plan sum the chunk's sizes (or only meet, so that no band reuses buffers
// another still reads), then the rate controller learns from the chunk
template <typename T> int finish_rate(mihevc_session *s, const Chunk<T> &c)
{
    const bool rc = s->rc.rc_on;
    if (c.halo.on && rc) {        // the sizes and estimates of every picture of the chunk, summed over the slices
        std::vector<size_t> idx((size_t)c.n);
        std::iota(idx.begin(), idx.end(), (size_t)c.first_index);
        if (int e = slice_sums(s, idx, true)) return e;
    } else if (c.halo.on) {
        if (!s->group->barrier()) return fail(s, kPeerFailed);
    }
    if (!rc) return 0;
    std::vector<std::vector<FrameRec>> lanes((size_t)c.gops);
    for (int g = 0; g < c.gops; g++) lanes[(size_t)g] = lane_records<T>(s, c, g, c.gl.glen[(size_t)g]);
    s->rc.learn(lanes);
    return 0;
}

void wait_all_jobs(mihevc_session *s)
{
    std::unique_lock<std::mutex> l(s->m);
    s->cv.wait(l, [&] { int n = 0; for (int g = 0; g < kGroups; g++) for (int k = 0; k < kRing; k++) n += s->slot[g][k].jobs_open; return n == 0; });
}

// the pending pictures as closed GOPs in lock-step: step t launches each stage once for picture t of every GOP
template <typename T> int encode_chunk(mihevc_session *s)
{
    const int n = (int)s->pending.size();
    if (!n) return 0;
    const auto wall0 = std::chrono::steady_clock::now();      // stats.reserved[3..5]: host time of the chunk in front of its first launch / behind its last kernel / in all (us, summed)
    GopLayout gl;
    if (int e = gop_layout<T>(s, n, gl)) return e;
    Chunk<T> c(s, n, std::move(gl));
    if (int e = ensure_lanes(s, c.gops)) return e;
    if (int e = setup_halo(s, c.gops, c.steps, c.halo)) return e;
    c.bf = s->cfg.bframes > 0;
    if (s->cfg.bframes < 0) { if (int e = probe_bframes<T>(s, n, c.bf)) return e; }
    // slices that exchange rows: their announcements are ordered by one global step; another session on the device: see open_sessions
    c.groups = c.halo.on || open_sessions(s->device).load() > 1 ? 1 : s->lane_groups;
    if (int e = alloc_chunk<T>(s, c)) return e;
    { std::lock_guard<std::mutex> l(s->m); s->frames.resize((size_t)s->frames_in); s->quality.resize((size_t)s->frames_in); }
    // every step's argument blocks, uploaded once
    for (int t = 0; t < c.steps; t++)
        for (int g = 0; g < c.gl.batch[(size_t)t]; g++) build_step_args<T>(s, c, t, g);
    HIPCK(s, hipMemcpyAsync(c.da, c.ha, c.need, hipMemcpyHostToDevice, s->st_compute));
    if (c.halo.on) HIPCK(s, hipMemcpyAsync(c.halo.dj, c.halo.hj, (size_t)c.steps * c.halo.jl.total, hipMemcpyHostToDevice, s->st_compute));
    s->rc.begin_chunk(c.bf, c.gl.glen);
    // ---- lock-step over the GOPs
    HIPCK(s, hipEventRecord(s->t_begin, s->st_compute));
    const auto wall1 = std::chrono::steady_clock::now();
    // Step 0 is one launch sequence for all lanes (the IDR decision reads every lane).  From step 1 on each lane group runs its own sequence on its own
    // stream, group 0 then group 1 for every t: a blocking wait for one group's step t - 2 always has the other group's work queued behind it, and the
    // device fills one sequence's launch tails and boundaries with the other's workgroups.
    bool second = false;      // lane group 1 has work on st_pre
    for (int t = 0; t < c.steps; t++)
        for (int grp = 0; grp < (t == 0 ? 1 : c.groups); grp++) {
            const Part p = c.part(s, grp, t);
            if (!p.n) continue;      // (a step with one lane left is group 0's alone)
            if (grp == 1 && !second) {      // group 1's first step: behind step 0 (compute stream); the search centres come down its own stream
                HIPCK(s, hipStreamWaitEvent(p.st, s->slot[0][0].compute, 0));
                second = true;
            }
            if (grp == 1) s->stats.reserved[6]++;      // steps that ran as two sequences
            {   // the slot this step writes must have been drained by its previous CABAC jobs
                std::unique_lock<std::mutex> l(s->m); s->cv.wait(l, [&] { return s->slot[p.grp][c.slot_of(t)].jobs_open == 0; });
            }
            if (int e = rate_feedback<T>(s, c, p, t)) return e;
            std::vector<int> qp_step((size_t)p.n);
            const bool history = s->rc.rc_on && type_of_step(c.bf, t) == 1;      // the P controller reads the lane's earlier pictures
            for (int k = 0; k < p.n; k++) {
                const int g = p.lanes[(size_t)k];
                qp_step[(size_t)k] = s->rc.step_qp(g, t, history ? lane_records<T>(s, c, g, t) : std::vector<FrameRec>());
                patch_qp<T>(s, c, t, g, qp_step[(size_t)k]);
            }
            if (int e = t == 0 ? idr_step<T>(s, c, qp_step) : inter_step<T>(s, c, p, t)) return e;
            if (int e = filter_and_copy<T>(s, c, p, t)) return e;
            hand_out<T>(s, c, p, t, qp_step);
        }
    if (second) {      // the chunk's device time ends when both groups have
        HIPCK(s, hipEventRecord(s->ev_join, s->st_pre));
        HIPCK(s, hipStreamWaitEvent(s->st_compute, s->ev_join, 0));
    }
    HIPCK(s, hipEventRecord(s->t_end, s->st_compute));
    HIPCK(s, hipStreamSynchronize(s->st_compute));
    const auto wall2 = std::chrono::steady_clock::now();
    HIPCK(s, hipStreamSynchronize(s->st_copy));
    HIPCK(s, hipStreamSynchronize(s->st_pre));        // a chunk without P steps never waited for its pre-search: its buffers are reused by the next chunk
    float ms = 0;
    (void)hipEventElapsedTime(&ms, s->t_begin, s->t_end);
    s->stats.device_ms += ms;
    for (auto &mk : s->marks) {
        float e = 0;
        if (hipEventElapsedTime(&e, s->ev_pool[mk.ev], s->ev_pool[mk.ev + 1]) == hipSuccess) {
            s->stats.stage_ms[mk.stage] += e; s->stats.stage_launches[mk.stage]++; s->stats.stage_pictures[mk.stage] += mk.pictures;
        }
    }
    s->marks.clear();
    wait_all_jobs(s);                                 // all CABAC jobs of the chunk
    s->gstep += c.steps;
    if (int e = finish_rate<T>(s, c)) return e;
    for (auto &src : s->pending) if (!src.borrowed) s->free_src.push_back(std::move(src));
    s->pending.clear();
    const auto wall3 = std::chrono::steady_clock::now();
    auto us = [](auto a, auto b) { return (int32_t)std::chrono::duration_cast<std::chrono::microseconds>(b - a).count(); };
    s->stats.reserved[3] += us(wall0, wall1); s->stats.reserved[4] += us(wall2, wall3); s->stats.reserved[5] += us(wall0, wall3);
    return 0;
}

int run_chunk(mihevc_session *s)
{
    if (hipSetDevice(s->device) != hipSuccess) return MIHEVC_EDEVICE;
    if (s->up_pending) {       // frames still on their way up (mihevc_send_frame_async, device-to-device copies): everything the chunk launches comes behind them
        HIPCK(s, hipEventRecord(s->ev_up, s->st_pre));
        HIPCK(s, hipStreamWaitEvent(s->st_compute, s->ev_up, 0));
        HIPCK(s, hipStreamWaitEvent(s->st_pre, s->ev_up, 0));
        s->up_pending = false;
    }
    return s->is16 ? encode_chunk<uint16_t>(s) : encode_chunk<uint8_t>(s);
}

}  // namespace

// a source picture whose planes are filled (or on their way on st_pre): pts bookkeeping, and the chunk once it is complete
int enqueue_source(mihevc_session *s, Src &&src, int64_t pts)
{
    src.pts = pts;
    if (s->frames_in == 0) s->first_pts = pts; else if (s->frames_in == 1) s->pts_step = std::max<int64_t>(1, pts - s->first_pts);
    s->pending.push_back(std::move(src));
    s->frames_in++;
    s->stats.frames_in = s->frames_in;
    if ((int)s->pending.size() >= s->lanes * s->keyint) return run_chunk(s);
    return MIHEVC_OK;
}

extern "C" {

int mihevc_open(const mihevc_config *cfg, int device, mihevc_session **out)
{
    if (!cfg || !out) return MIHEVC_EINVAL;
    *out = nullptr;
    if (cfg->width < 16 || cfg->height < 16 || (cfg->width & 1) || (cfg->height & 1) || cfg->width > 8192 || cfg->height > 4352) return MIHEVC_EINVAL;
    if (cfg->bit_depth != 8 && cfg->bit_depth != 10) return MIHEVC_EINVAL;
    if (cfg->sign_hide != 0 && cfg->sign_hide != 1) return MIHEVC_EINVAL;
    if (cfg->pic_hash < 0 || cfg->pic_hash > 3 || (cfg->pic_hash && cfg->slice_count > 1)) return MIHEVC_EINVAL;      // hashes of sliced pictures: not yet
    if ((cfg->ssim != 0 && cfg->ssim != 1) || (cfg->ssim && cfg->slice_count > 1)) return MIHEVC_EINVAL;      // windows cross the seams; a band sees only its rows
    if (cfg->fps_num <= 0 || cfg->fps_den <= 0 || cfg->keyint < 1 || cfg->keyint > 240) return MIHEVC_EINVAL;
    if (cfg->bframes < -1 || cfg->bframes > 1 || (cfg->bframes && cfg->slice_count > 1)) return MIHEVC_EINVAL;      // B pictures: whole pictures only (for now)
    if (cfg->slice_count > 1) {        // one slice of a picture: a band of whole CTU rows (the last band takes the picture's remainder)
        if (cfg->slice_count > 16 || cfg->slice_index < 0 || cfg->slice_index >= cfg->slice_count || cfg->pic_height < cfg->height) return MIHEVC_EINVAL;
        int rows = 0;
        for (int k = 0; k < cfg->slice_count; k++) { if (cfg->slice_ctu_rows[k] < 1) return MIHEVC_EINVAL; rows += cfg->slice_ctu_rows[k]; }
        if (rows != (cfg->pic_height + 31) / 32) return MIHEVC_EINVAL;
        const int y0 = 32 * slice_first_row(*cfg, cfg->slice_index), y1 = std::min(cfg->pic_height, y0 + 32 * cfg->slice_ctu_rows[cfg->slice_index]);
        if (cfg->height != y1 - y0) return MIHEVC_EINVAL;
    }
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return MIHEVC_ENODEV;
    if (device < 0 || device >= n) return MIHEVC_EINVAL;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return MIHEVC_EDEVICE;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return MIHEVC_ENODEV;      // the code objects are gfx950 only
    if (hipSetDevice(device) != hipSuccess) return MIHEVC_EDEVICE;
    mihevc_session *s = new (std::nothrow) mihevc_session();
    if (!s) return MIHEVC_ENOMEM;
    s->cfg = *cfg;
    if (s->cfg.sao < 0) s->cfg.sao = 1;
    s->device = device;
    open_sessions(device)++;      // (mihevc_close takes it back, on the failure paths below too)
    CodedSize cs = coded_size(cfg->width, cfg->height);
    s->w = cs.w; s->h = cs.h;
    s->ctus_w = (s->w + CTU - 1) / CTU; s->ctus_h = (s->h + CTU - 1) / CTU; s->n_ctu = s->ctus_w * s->ctus_h;
    s->tiles = tile_grid(s->cfg);
    s->ptiles = p_tile_grid(s->cfg);
    s->ring = cfg->level_idc >= 150 ? kRing : 8;
    s->is16 = cfg->bit_depth > 8;
    s->keyint = cfg->keyint;
    s->lanes = cfg->gops_in_flight > 0 ? std::min(cfg->gops_in_flight, MAX_LANES) : 4;
    // A/B switch: MIHEVC_LANE_GROUPS=1 runs the P/B steps of a chunk as one launch sequence on the compute stream; the stream is the same either way
    if (const char *e = getenv("MIHEVC_LANE_GROUPS")) s->lane_groups = atoi(e) == 1 ? 1 : kGroups;
    s->me_range = cfg->me_range > 0 ? std::min(cfg->me_range, MAX_RANGE) : 15;   // 8 quads x 31 rows = 248 items: one pass of the 256-thread search
    // constant-quality operating point: P pictures at crf + 2, IDR pictures 3 below (x265's ipratio 1.4 ~ 3 QP)
    s->qp_p = cfg->qp >= 0 ? cfg->qp : std::min(51, std::max(0, cfg->crf + 2));
    s->qp_i = std::max(0, s->qp_p - 3);
    s->stats.last_qp = s->qp_p;
    write_parameter_sets(s->cfg, s->headers);
    bool ok = s->events_ok() && s->st_compute.acquire(device) == hipSuccess && s->st_copy.acquire(device) == hipSuccess && s->st_pre.acquire(device) == hipSuccess;
    if (ok && cfg->pic_hash >= 2) ok = s->hash_part.alloc(device, (size_t)MAX_LANES * pic_hash_part_words(s->w, s->h, (int)esize(s)) * sizeof(uint32_t), false) == hipSuccess;
    if (ok && cfg->ssim) ok = s->ssim_part.alloc(device, (size_t)MAX_LANES * ssim_part_words(s->w, s->h) * sizeof(long long), false) == hipSuccess;
    if (!ok) { mihevc_close(s); return MIHEVC_EDEVICE; }      // gives back what was acquired
    if (cfg->slice_count > 1 && cfg->slice_halo) {
        // one slice of a picture whose slices exchange rows: meet the others (csrc/slice_group.h), and get the buffers the neighbours read
        s->n_bands = cfg->slice_count; s->band = cfg->slice_index;
        for (int k = 0, y0 = 0; k < cfg->slice_count; k++) {
            const int y1 = std::min(cfg->pic_height, y0 + 32 * cfg->slice_ctu_rows[k]);
            s->band_h[k] = coded_size(cfg->width, y1 - y0).h;
            y0 = y1;
        }
        const size_t es = s->is16 ? 2 : 1;
        s->x1_part_bytes = (((size_t)kSeamRows * s->w + (size_t)kSeamRows * (s->w / 2)) * es + (size_t)(s->w >> 3) * sizeof(mihevc_cu_rec) + 255) & ~(size_t)255;
        s->x1_lane_bytes = 2 * s->x1_part_bytes;
        for (int k = 0; ok && k < 2; k++) {
            s->ev_x1[k] = Event(hipEventDisableTiming); s->ev_x2[k] = Event(hipEventDisableTiming);
            ok = s->x1_export[k].alloc(device, s->x1_lane_bytes * kHaloLanes, false) == hipSuccess && s->ev_x1[k] && s->ev_x2[k];
        }
        if (!ok || cfg->slice_group == 0) { mihevc_close(s); return cfg->slice_group == 0 ? MIHEVC_EINVAL : MIHEVC_EDEVICE; }
        s->group = SliceGroup::join(cfg->slice_group, cfg->slice_count);
    }
    // a slice of a picture (one device of several) plans with its share of the picture's rate and buffer
    // (slices that share one rate plan — cfg.slice_halo — plan the whole picture's rate from inputs summed over the slices)
    const double share = s->group ? 1.0 : (cfg->slice_count > 1 && cfg->rate_share_q16 > 0) ? cfg->rate_share_q16 / 65536.0 : 1.0;
    s->rc.init(s->cfg, s->qp_i, s->qp_p, share, s->ring - 1);      // a P step's CABAC job is complete once its ring slot has been handed out again
    int threads = cfg->host_threads > 0 ? cfg->host_threads : (int)std::min(16u, std::max(2u, std::thread::hardware_concurrency()));
    s->pool = &ThreadPool::shared(threads);
    s->host_threads = threads;
    *out = s;
    return MIHEVC_OK;
}

int mihevc_sync_uploads(mihevc_session *s)
{
    if (!s) return MIHEVC_EINVAL;
    if (s->failed) return s->fail_code;
    if (hipSetDevice(s->device) != hipSuccess) return MIHEVC_EDEVICE;
    HIPCK(s, hipStreamSynchronize(s->st_pre));
    s->up_pending = false;
    return MIHEVC_OK;
}

int mihevc_flush(mihevc_session *s)
{
    if (!s) return MIHEVC_EINVAL;
    if (s->failed) return s->fail_code;
    if (s->flushed) return MIHEVC_OK;
    if (int e = source_flush(s)) return e;      // the last frame of a ring: its successor is itself
    s->flushing = true;
    int e = run_chunk(s);
    s->flushed = true;
    return e;
}

int mihevc_abort(mihevc_session *s)
{
    if (!s) return MIHEVC_EINVAL;
    { std::lock_guard<std::mutex> l(s->m); if (s->err.empty()) s->err = "aborted by the caller"; }
    s->failed = true;
    if (s->group) s->group->fail();
    return MIHEVC_OK;
}

int mihevc_receive_packet(mihevc_session *s, const uint8_t **data, size_t *size, int64_t *pts, int64_t *dts, int *keyframe)
{
    if (!s || !data || !size) return MIHEVC_EINVAL;
    s->cur_batch.clear();
    std::unique_lock<std::mutex> l(s->m);
    auto it = s->packets.find(s->next_out);
    if (it == s->packets.end() || !it->second.ready) return (s->flushed && s->next_out >= s->frames_in) ? MIHEVC_EOF : MIHEVC_EAGAIN;
    if (!it->second.error.empty()) { std::string err = it->second.error; l.unlock(); s->fail_code = MIHEVC_EINVAL; fail(s, err); return MIHEVC_EINVAL; }
    s->cur_packet = std::move(it->second.data);
    if (pts) *pts = it->second.pts;
    if (dts) *dts = it->second.dts;        // packets come in decoding order; dts < pts only with B pictures (cfg.bframes)
    if (keyframe) *keyframe = it->second.key;
    s->packets.erase(it);
    s->next_out++;
    s->stats.frames_out = s->next_out;
    *data = s->cur_packet.data();
    *size = s->cur_packet.size();
    return MIHEVC_OK;
}

// mihevc_receive_packet up to `max` times under one lock: the packets move out of the map into cur_batch, which owns them until the next receive call
int mihevc_receive_packets(mihevc_session *s, int max, const uint8_t **data, size_t *size, int64_t *pts, int64_t *dts, int *keyframe)
{
    if (!s || max <= 0 || !data || !size) return MIHEVC_EINVAL;
    s->cur_batch.clear();
    std::unique_lock<std::mutex> l(s->m);
    int n = 0;
    auto it = s->packets.find(s->next_out);
    while (n < max && it != s->packets.end() && it->first == s->next_out && it->second.ready) {
        if (!it->second.error.empty()) {
            if (n) break;      // the packets in front of it go out first; the next call fails as the one-packet form does
            std::string err = it->second.error; l.unlock(); s->fail_code = MIHEVC_EINVAL; fail(s, err); return MIHEVC_EINVAL;
        }
        s->cur_batch.push_back(std::move(it->second.data));
        data[n] = s->cur_batch.back().data();
        size[n] = s->cur_batch.back().size();
        if (pts) pts[n] = it->second.pts;
        if (dts) dts[n] = it->second.dts;
        if (keyframe) keyframe[n] = it->second.key;
        it = s->packets.erase(it);
        s->next_out++;
        n++;
    }
    if (!n) return (s->flushed && s->next_out >= s->frames_in) ? MIHEVC_EOF : MIHEVC_EAGAIN;
    s->stats.frames_out = s->next_out;
    return n;
}

int mihevc_get_headers(mihevc_session *s, const uint8_t **data, size_t *size)
{
    if (!s || !data || !size) return MIHEVC_EINVAL;
    *data = s->headers.data();
    *size = s->headers.size();
    return MIHEVC_OK;
}

int mihevc_get_stats(const mihevc_session *s, mihevc_stats *out)
{
    if (!s || !out) return MIHEVC_EINVAL;
    std::lock_guard<std::mutex> l(const_cast<mihevc_session *>(s)->m);
    *out = s->stats;
    out->entropy_ms = (double)s->entropy_ns.load() / 1e6;
    double *ssim[3] = {&out->ssim_y, &out->ssim_u, &out->ssim_v};
    for (int c = 0; c < 3; c++) *ssim[c] = s->cfg.ssim ? (double)s->ssim_total[c] / ((double)ssim_window_count(s, c) * 4294967296.0) : 0.0;
    return MIHEVC_OK;
}

int mihevc_set_keep_recon(mihevc_session *s, int keep)
{
    if (!s) return MIHEVC_EINVAL;
    s->keep_recon = keep != 0;
    return MIHEVC_OK;
}

int mihevc_get_recon(mihevc_session *s, int64_t index, uint16_t *y, uint16_t *u, uint16_t *v)
{
    if (!s || !y || !u || !v) return MIHEVC_EINVAL;
    auto it = s->recon.find(index);
    if (it == s->recon.end()) return MIHEVC_ESTATE;
    size_t ny = (size_t)s->w * s->h;
    memcpy(y, it->second.data(), ny * 2);
    memcpy(u, it->second.data() + ny, ny / 2);
    memcpy(v, it->second.data() + ny + ny / 4, ny / 2);
    return MIHEVC_OK;
}

int mihevc_get_frame_info(mihevc_session *s, int64_t index, int *qp, int *slice_type, int64_t *bits)
{
    if (!s) return MIHEVC_EINVAL;
    std::lock_guard<std::mutex> l(s->m);
    if (index < 0 || (size_t)index >= s->frames.size()) return MIHEVC_ESTATE;
    const auto &fr = s->frames[(size_t)index];
    if (qp) *qp = fr.qp;
    if (slice_type) *slice_type = fr.type;
    if (bits) *bits = fr.bits;
    return MIHEVC_OK;
}

int mihevc_get_frame_quality(mihevc_session *s, int64_t index, uint64_t sse[3], int64_t ssim_q32[3], int64_t ssim_windows[3])
{
    if (!s) return MIHEVC_EINVAL;
    if ((ssim_q32 || ssim_windows) && !s->cfg.ssim) return MIHEVC_ESTATE;
    std::lock_guard<std::mutex> l(s->m);
    if (index < 0 || (size_t)index >= s->quality.size()) return MIHEVC_ESTATE;
    const auto &q = s->quality[(size_t)index];
    if (!q.known) return MIHEVC_EAGAIN;
    for (int c = 0; c < 3; c++) {
        if (sse) sse[c] = q.sse[c];
        if (ssim_q32) ssim_q32[c] = q.ssim[c];
        if (ssim_windows) ssim_windows[c] = ssim_window_count(s, c);
    }
    return MIHEVC_OK;
}

int mihevc_coded_size(const mihevc_session *s, int *w, int *h)
{
    if (!s || !w || !h) return MIHEVC_EINVAL;
    *w = s->w; *h = s->h;
    return MIHEVC_OK;
}

const char *mihevc_last_error(const mihevc_session *s) { return s ? s->err.c_str() : host_last_error(); }

void mihevc_close(mihevc_session *s)
{
    if (!s) return;
    (void)hipSetDevice(s->device);
    wait_all_jobs(s);           // the session's CABAC jobs still in flight (an abandoned session): they hold pointers into it
    if (s->st_compute) (void)hipStreamSynchronize(s->st_compute);
    if (s->st_copy) (void)hipStreamSynchronize(s->st_copy);
    if (s->st_pre) (void)hipStreamSynchronize(s->st_pre);
    open_sessions(s->device)--;
    delete s;                   // every buffer, event and stream goes back through its handle; the streams are idle (synchronised above)
}

}  // extern "C"
