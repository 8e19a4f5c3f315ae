// hevc_amd/csrc/source.cpp — the source front end of a session: every mihevc_send_frame* entry, from the caller's picture in any layout through
// any filter to enqueue_source, all on st_pre.  It meets the encoder proper (session.cpp) at take_src, at finish_ingest / enqueue_source and at source_flush; its
// state is mihevc_session::src (session.h).  A converting entry is written against convert_frame: it describes the caller's planes and hands over a callable that
// builds the kernel's arguments and launches it; the device, the set of planes, the staging of host planes and the hand-over to the session are the frame's.
#include <cstring>
#include <utility>

#include "chain_plan.h"
#include "fieldmatch_plan.h"
#include "session.h"

namespace {

// where the caller's planes are and when the call returns: MIHEVC_SRC_DEVICE and MIHEVC_SRC_ASYNC of the converting entries, decoded once
struct SrcFlags {
    bool device, async;
    static SrcFlags of(int flags) { return {(flags & MIHEVC_SRC_DEVICE) != 0, (flags & MIHEVC_SRC_ASYNC) != 0}; }
    bool wait() const { return !device && !async; }
};

// the planes a source picture is written to: a set the last chunk gave back, or new ones (a failure midway: `src` gives back the planes it had taken)
int take_src(mihevc_session *s, Src &src)
{
    if (!s->free_src.empty()) { src = std::move(s->free_src.back()); s->free_src.pop_back(); }
    else if (int e = alloc_planes(s, src.mem, src.p, src.stride, 0)) return e;
    src.borrowed = false;
    return MIHEVC_OK;
}

// Uploads and conversions run on st_pre; the chunk's first launch waits for the event behind the last one.  wait: the synchronous entry points of host planes
// wait here (the caller may reuse its buffers on return), the others return with the work in flight
int finish_ingest(mihevc_session *s, Src &&src, int64_t pts, bool wait)
{
    if (wait) HIPCK(s, hipStreamSynchronize(s->st_pre));
    else s->up_pending = true;
    return enqueue_source(s, std::move(src), pts);
}

// a plane of a source on its way to a converter: row and pitch in elements
struct SrcPlane { const void *p; int row, rows, pitch; };
// Host planes go through the staging set: laid out one behind the other with rows that begin 16-byte aligned (the kernels' widest loads), copied on st_pre;
// p and pitch of every plane then name its copy.  Device planes stay where they are
int stage_planes(mihevc_session *s, SrcPlane *pl, int n, size_t es, bool device_src)
{
    if (device_src) return MIHEVC_OK;
    CachedBlock<uint8_t> &stage = s->src.stage;
    size_t off[3], total = 0;
    int spitch[3];
    for (int c = 0; c < n; c++) {
        spitch[c] = (pl[c].row + 15) & ~15;
        off[c] = total;
        total += ((size_t)spitch[c] * pl[c].rows * es + 255) & ~(size_t)255;
    }
    if (total > stage.bytes()) {
        HIPCK(s, hipStreamSynchronize(s->st_pre));      // a conversion still reading the smaller set
        HIPCK(s, stage.alloc(s->device, total, false));
    }
    for (int c = 0; c < n; c++) {
        HIPCK(s, hipMemcpy2DAsync(stage + off[c], spitch[c] * es, pl[c].p, pl[c].pitch * es, pl[c].row * es, pl[c].rows, hipMemcpyHostToDevice, s->st_pre));
        pl[c].p = stage + off[c]; pl[c].pitch = spitch[c];
    }
    return MIHEVC_OK;
}

// The conversion frame of every converting entry (the arguments are checked): the device, a set of planes, the caller's n planes `pl` of es-byte elements through
// the staging set, launch(src, pl) (it builds the kernel's arguments from the staged planes and launches on st_pre), the hand-over.  A failure after take_src has
// gone through fail(): the session is failed for good, and `src` lets go of its planes on the way out, into the process-wide cache, not back into free_src
template <typename Launch> int convert_frame(mihevc_session *s, SrcFlags fl, int64_t pts, SrcPlane *pl, int n, size_t es, Launch &&launch)
{
    if (hipSetDevice(s->device) != hipSuccess) return MIHEVC_EDEVICE;
    Src src;
    if (int e = take_src(s, src)) return e;
    if (int e = stage_planes(s, pl, n, es, fl.device)) return e;
    if (int e = launch(src, pl)) return e;
    return finish_ingest(s, std::move(src), pts, fl.wait());
}

// may_borrow: device planes that need no margin may be coded where they are (the rule of mihevc_send_frame_device: valid until the packet is out); false: always copied,
// so the caller's planes are free once the uploads are through (the rule of mihevc_send_frame_fmt)
int ingest(mihevc_session *s, const void *y, const void *u, const void *v, int pitch_y, int pitch_c, int64_t pts, SrcFlags fl, bool may_borrow = true)
{
    if (!s || !y || !u || !v) return MIHEVC_EINVAL;
    if (s->failed) return s->fail_code;
    if (s->flushed || s->src.ring.pending || s->src.fm.open || s->src.chain.set) return MIHEVC_ESTATE;      // (a deinterlaced or denoised frame waits for its successor: no other picture may come between; fieldmatch cycles are not interleaved)
    if (hipSetDevice(s->device) != hipSuccess) return MIHEVC_EDEVICE;
    Src src;
    const void *in[3] = {y, u, v};
    const size_t es = esize(s);
    // Device planes whose size already is the coded size (no margin to fill) are used where they are: the header's contract keeps them valid and
    // unmodified until the picture's packet is out.  Saves three 2-D copies per frame (4 % of the device time of a 1080p clip, and most of the
    // wall time of handing 300 frames over).
    if (may_borrow && fl.device && s->cfg.width == s->w && s->cfg.height == s->h && pitch_y >= s->w && pitch_c >= s->w / 2 &&
        ((uintptr_t)y & 3) == 0 && ((uintptr_t)u & 3) == 0 && ((uintptr_t)v & 3) == 0 && (pitch_y * es) % 4 == 0 && (pitch_c * es) % 4 == 0) {
        for (int i = 0; i < 3; i++) { src.p[i] = const_cast<void *>(in[i]); src.stride[i] = i ? pitch_c : pitch_y; }
        src.borrowed = true;
        return enqueue_source(s, std::move(src), pts);
    }
    if (int e = take_src(s, src)) return e;
    for (int i = 0; i < 3; i++) {
        int pw = i ? s->w / 2 : s->w, ph = i ? s->h / 2 : s->h;               // coded plane size
        int sw = i ? s->cfg.width / 2 : s->cfg.width, sh = i ? s->cfg.height / 2 : s->cfg.height, pitch = i ? pitch_c : pitch_y;
        if (pitch < sw) return MIHEVC_EINVAL;
        HIPCK(s, hipMemcpy2DAsync(src.p[i], src.stride[i] * es, in[i], pitch * es, sw * es, sh, fl.device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s->st_pre));
        // replicate the last column/row into the coded-size margin (the conformance window crops it again)
        if (pw > sw || ph > sh) {
            if (s->is16) HIPCK(s, launch_extend_margin<uint16_t>(s->st_pre, Plane<uint16_t>{(uint16_t *)src.p[i], src.stride[i]}, sw, sh, pw, ph));
            else HIPCK(s, launch_extend_margin<uint8_t>(s->st_pre, Plane<uint8_t>{(uint8_t *)src.p[i], src.stride[i]}, sw, sh, pw, ph));
        }
    }
    return finish_ingest(s, std::move(src), pts, fl.wait());
}

// matrix and range of an R'G'B' source: the format's own, else the session's.  fmt_ok false: matrix 0, which no entry accepts
struct RgbColour { int matrix; bool full; };
RgbColour rgb_colour(const mihevc_session *s, const mihevc_rgb_format *fmt, bool fmt_ok)
{
    return {!fmt_ok ? 0 : fmt->matrix ? fmt->matrix : s->cfg.matrix, fmt_ok && (fmt->range ? fmt->range == 2 : s->cfg.full_range != 0)};
}

using Ring = SourceFront::Ring;

// What a ring stage writes its pictures to, and what becomes of them.  take: the planes of the next picture and the coded size to fill; put: its
// kernel is launched (pts: what the stage's own entry would number it); drop: it will not go on (decimation)
struct Sink {
    virtual int take(Out &o) = 0;
    virtual int put(Out &&o, int64_t pts) = 0;
    virtual void drop(Out &&o) = 0;
protected:
    ~Sink() = default;
};
// the sink of the single entries: a Src of the session, handed to the encoder with the stage's pts
struct SrcSink final : Sink {
    mihevc_session *s; bool wait;
    SrcSink(mihevc_session *s_, bool wait_) : s(s_), wait(wait_) {}
    int take(Out &o) override
    {
        if (int e = take_src(s, o.src)) return e;
        for (int c = 0; c < 3; c++) { o.p[c] = o.src.p[c]; o.stride[c] = o.src.stride[c]; }
        o.pw = s->w; o.ph = s->h;
        return MIHEVC_OK;
    }
    int put(Out &&o, int64_t pts) override { return finish_ingest(s, std::move(o.src), pts, wait); }
    void drop(Out &&o) override { s->free_src.push_back(std::move(o.src)); }
};

// Frame k of the ring produces its picture(s): P = frame k - 1 (the first frame: itself), C = frame k, N = frame k + 1 (has_next; the last frame: itself)
struct RingFrames { void *const *P, *const *C, *const *N; };
RingFrames ring_take(Ring &r, int64_t k, bool has_next)
{
    r.pending = false;
    return {r.p[(k > 0 ? k - 1 : k) % 3], r.p[k % 3], r.p[(has_next ? k + 1 : k) % 3]};
}

// The picture(s) of frame k of ring r (mihevc_send_frame_deint, mihevc_send_frame_denoise, a chain's stages): P, C, N as ring_take.  k_deint / k_denoise /
// k_mcfi_render write the planes the sink names, margin included, out of the ring, at the ring's size and depth.  Deinterlacing: frame-rate mode keeps the first
// field's rows, field-rate mode follows with the second field's picture at pts + 1.  Denoising: one picture, with the strengths frame k came with.  Interpolation
// (mihevc_send_frame_interpolate): the vectors of the pair (C, N), then `factor` pictures at pts + j; the last frame: its own picture only
int ring_emit(mihevc_session *s, Ring &r, int64_t k, bool has_next, Sink &sink)
{
    const auto [P, C, N] = ring_take(r, k, has_next);
    const bool denoise = r.kind == SourceFront::RING_DENOISE, is16 = r.depth > 8;
    const int W = r.w, H = r.h;
    if (r.kind == SourceFront::RING_MCFI) {      // the pictures between C and N; the last frame: itself (picture 0 of a blend with any N)
        mihevc_interpolate m = s->src.mcfi.pending;
        if (!has_next) m.mode = 1;
        const McfiLayout l = mcfi_layout(W, H);
        uint8_t *const blk = s->src.mcfi.dev.get();
        if (m.mode == 0) {
            const McfiSearchArgs a = mcfi_search_args(r.depth, C[0], N[0], r.pitch[0], W, H, blk);
            HIPCK(s, launch_mcfi_vectors(s->st_pre, a, mcfi_field_args(a, blk), is16));
        }
        for (int j = 0; j < (has_next ? m.factor : 1); j++) {
            Out o;
            if (int e = sink.take(o)) return e;
            const McfiRenderArgs a = mcfi_render_args(m, j, r.depth, C, N, r.pitch[0], r.pitch[1], W, H, o.pw, o.ph, (const int16_t *)(blk + l.v),
                                                      (const unsigned long long *)(blk + l.dsum), o.p, o.stride);
            HIPCK(s, launch_mcfi_render(s->st_pre, a, is16));
            if (int e = sink.put(std::move(o), r.pts + j)) return e;
        }
        return MIHEVC_OK;
    }
    const int first = r.deint_tff ? 0 : 1;
    for (int f = 0; f <= (denoise ? 0 : r.deint_field_rate); f++) {
        Out o;
        if (int e = sink.take(o)) return e;
        if (denoise) {
            const DenoiseArgs a = denoise_args(r.denoise_pending, r.depth, P, C, N, r.pitch[0], r.pitch[1], W, H, o.pw, o.ph, o.p, o.stride);
            HIPCK(s, launch_denoise(s->st_pre, a, is16));
        } else {
            const DeintArgs a = deint_args(r.depth, P, C, N, r.pitch[0], r.pitch[1], W, H, o.pw, o.ph, f ? 1 - first : first, f, o.p, o.stride);
            HIPCK(s, launch_deint(s->st_pre, a, is16));
        }
        if (int e = sink.put(std::move(o), r.pts + f)) return e;
    }
    return MIHEVC_OK;
}

// decimate: the held pictures go on in order, all but the one at `drop` (-1: a partial cycle comes out whole), which goes back to its sink
int fm_release(mihevc_session *s, int drop, Sink &sink)
{
    SourceFront::Fm &fm = s->src.fm;
    auto held = std::move(fm.held);
    fm.held.clear();
    int e = MIHEVC_OK;
    for (size_t i = 0; i < held.size(); i++) {
        const bool dropped = (int)i == drop;
        {
            std::lock_guard<std::mutex> l(s->m);
            auto &f = fm.frames[(size_t)held[i].second];
            f.info.dropped = dropped; f.info.picture = dropped || e ? -1 : fm.pictures; f.decided = true;
        }
        if (dropped || e) { sink.drop(std::move(held[i].first)); continue; }
        e = sink.put(std::move(held[i].first), fm.first_pts + fm.pictures++);
    }
    return e;
}

// Frame k of ring r is decided (mihevc_send_frame_fieldmatch, a chain's field stage): P, C, N as ring_take.  The metrics of the frame are taken on
// st_pre and copied to pinned memory behind fm.ev; the host waits for that event only, plans (csrc/fieldmatch_plan.h) and launches the weave, or the
// deinterlacer, into the planes the sink names.  Without decimate the picture goes on with its frame's pts; with it the picture is held until its cycle's fifth
// frame is decided
int fm_decide(mihevc_session *s, Ring &r, int64_t k, bool has_next, Sink &sink)
{
    SourceFront::Fm &fm = s->src.fm;
    const auto [P, C, N] = ring_take(r, k, has_next);
    const int W = r.w, H = r.h, keep = fm.mode.tff ? 0 : 1;
    const bool is16 = r.depth > 8;
    const size_t nwg = (size_t)fm_workgroups(W, H);
    unsigned long long *const part = (unsigned long long *)fm.dev.get(), *const host = (unsigned long long *)fm.host.get();
    HIPCK(s, launch_fm_metrics(s->st_pre, fm_args(r.depth, P[0], C[0], N[0], r.pitch[0], W, H, keep, part), part + nwg * 8, is16));
    HIPCK(s, hipMemcpyAsync(host, part + nwg * 8, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s->st_pre));
    HIPCK(s, hipEventRecord(fm.ev, s->st_pre));
    HIPCK(s, hipEventSynchronize(fm.ev));
    FmMetrics m = fm_metrics_of(host);
    if (k == 0) fm_first_frame(m);
    const int match = fm_match(m);
    const bool fallback = fm_falls_back(m, match, fm.mode.deint != 0);
    Out o;
    if (int e = sink.take(o)) return e;
    if (fallback) {
        const DeintArgs a = deint_args(r.depth, P, C, N, r.pitch[0], r.pitch[1], W, H, o.pw, o.ph, keep, 0, o.p, o.stride);
        HIPCK(s, launch_deint(s->st_pre, a, is16));
    } else {
        void *const *X = match == 0 ? C : match == 1 ? P : N;
        const DeintArgs a = deint_args(r.depth, X, C, X, r.pitch[0], r.pitch[1], W, H, o.pw, o.ph, keep, 0, o.p, o.stride);
        HIPCK(s, launch_fm_weave(s->st_pre, a, is16));
    }
    mihevc_fm_frame info = {};
    for (int i = 0; i < 3; i++) { info.comb_sum[i] = m.comb_sum[i]; info.comb_block[i] = m.comb_block[i]; }
    info.dup_sum = m.dup_sum; info.dup_block = m.dup_block; info.match = match; info.deinterlaced = fallback; info.dropped = 0;
    info.picture = fm.mode.decimate ? -1 : fm.pictures;
    {
        std::lock_guard<std::mutex> l(s->m);
        fm.frames[(size_t)k] = {info, !fm.mode.decimate};
    }
    if (!fm.mode.decimate) { fm.pictures++; return sink.put(std::move(o), r.pts); }
    fm.held.emplace_back(std::move(o), k);
    if ((int)fm.held.size() < kFmCycle) return MIHEVC_OK;
    FmMetrics cycle[kFmCycle] = {};
    for (int i = 0; i < kFmCycle; i++) {
        const mihevc_fm_frame &f = fm.frames[(size_t)fm.held[(size_t)i].second].info;
        cycle[i].dup_sum = f.dup_sum; cycle[i].dup_block = f.dup_block;
    }
    return fm_release(s, fm_drop(cycle), sink);
}

// A picture of w luma samples a row and `rows` rows at es bytes a sample in one block: rows that begin 16-byte aligned (pitches in samples), planes 256-byte
// aligned.  A ring's slot, a chain's hop picture
hipError_t picture_alloc(mihevc_session *s, CachedBlock<uint8_t> &mem, void *(&p)[3], int (&pitch)[3], int w, int rows, size_t es)
{
    pitch[0] = (w + 15) & ~15; pitch[1] = pitch[2] = (w / 2 + 15) & ~15;
    const size_t by = ((size_t)pitch[0] * rows * es + 255) & ~(size_t)255, bc = ((size_t)pitch[1] * (rows / 2) * es + 255) & ~(size_t)255;
    if (hipError_t e = mem.alloc(s->device, by + 2 * bc, false)) return e;
    p[0] = mem; p[1] = mem + by; p[2] = mem + by + bc;
    return hipSuccess;
}
// the three slots of a ring of w x h pictures at `depth`, of `rows` rows each
hipError_t ring_alloc(mihevc_session *s, Ring &r, int kind, int w, int h, int depth, int rows)
{
    for (int k = 0; k < 3; k++)
        if (hipError_t e = picture_alloc(s, r.mem[k], r.p[k], r.pitch, w, rows, depth > 8 ? 2 : 1)) return e;
    r.w = w; r.h = h; r.depth = depth; r.rows = rows; r.kind = kind;
    return hipSuccess;
}

// A frame of kind `kind` (mihevc_send_frame_deint, mihevc_send_frame_denoise; the arguments are checked): into its slot of the ring, then the picture(s) of the frame
// before it.  Returns with ring.pts still that of the frame before: the caller sets what belongs to the new frame
int ingest_ring(mihevc_session *s, int kind, const void *y, const void *u, const void *v, int pitch_y, int pitch_c, int64_t pts, SrcFlags fl)
{
    if (hipSetDevice(s->device) != hipSuccess) return MIHEVC_EDEVICE;
    Ring &r = s->src.ring;
    const size_t es = esize(s);
    const int W = s->cfg.width, H = s->cfg.height;
    if (!r.mem[0]) HIPCK(s, ring_alloc(s, r, kind, W, H, s->cfg.bit_depth, H));
    const int64_t k = r.n;
    const void *in[3] = {y, u, v};
    for (int c = 0; c < 3; c++)
        HIPCK(s, hipMemcpy2DAsync(r.p[k % 3][c], r.pitch[c] * es, in[c], (c ? pitch_c : pitch_y) * es, (c ? W / 2 : W) * es, c ? H / 2 : H,
                                  fl.device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s->st_pre));
    r.n = k + 1;
    const bool wait = fl.wait();
    SrcSink sink(s, wait);
    int e = MIHEVC_OK;
    if (k > 0) e = kind == SourceFront::RING_FIELDMATCH ? fm_decide(s, r, k - 1, true, sink) : ring_emit(s, r, k - 1, true, sink);      // (ring.pts and denoise_pending are still those of frame k - 1)
    else if (wait) HIPCK(s, hipStreamSynchronize(s->st_pre));
    else s->up_pending = true;
    r.pts = pts;
    r.pending = true;
    return e;
}

// What the converting entries refuse, in the order in which the errors win.  args_ok: the entry's own checks of its arguments
int refuse_source(const mihevc_session *s, bool args_ok, int flags, int kind = SourceFront::RING_NONE)
{
    if (!args_ok || (flags & ~(MIHEVC_SRC_DEVICE | MIHEVC_SRC_ASYNC))) return MIHEVC_EINVAL;
    if ((s->cfg.width & 1) || (s->cfg.height & 1) || s->cfg.slice_count > 1) return MIHEVC_EINVAL;      // (bands of a 4:2:2 picture: out of scope)
    if (s->failed) return s->fail_code;
    if (s->src.fm.open && kind != SourceFront::RING_FIELDMATCH) return MIHEVC_ESTATE;      // (from the first fieldmatch frame until flush)
    return s->flushed || s->src.chain.set || (s->src.ring.pending && s->src.ring.kind != kind) ? MIHEVC_ESTATE : MIHEVC_OK;      // (a chain: its own entry only)
}

// the intermediate picture of the resized route: planar 4:2:0 at 10 bit of the network's output size nw x nh, coded size rounded up to 8 as every coded
// picture's (scale x an even source at scale 4: its own size), rows 16-byte aligned.  Returns its bytes
size_t sr_mid_layout(int nw, int nh, size_t (&off)[3], int (&stride)[3], int &pw, int &ph)
{
    pw = (nw + 7) & ~7; ph = (nh + 7) & ~7;
    size_t n = 0;
    for (int c = 0; c < 3; c++) {
        stride[c] = ((c ? pw / 2 : pw) + 15) & ~15;
        off[c] = n;
        n += ((size_t)stride[c] * (c ? ph / 2 : ph) * sizeof(uint16_t) + 255) & ~(size_t)255;
    }
    return n;
}
// The session's size against (nw, nh) = scale x the source: 0 the direct route, 1 the resized route, -1 neither (the geometry rule of mihevc_send_frame_sr_yuv)
int sr_route(const mihevc_session *s, int nw, int nh)
{
    if (s->cfg.width == nw && s->cfg.height == nh) return 0;
    return scale_geometry_ok(nw, nh, s->cfg.width, s->cfg.height) ? 1 : -1;
}
// The session's model of either kind (mihevc_set_sr_model, mihevc_set_sr_compact; neither: no model) as sr_frame needs it.  A compact network has no
// pixel-unshuffle: its input tensor is the source at its own size at either scale
struct SrModelRef {
    const SrNet *net = nullptr;
    const SrCompactNet *cnet = nullptr;
    explicit SrModelRef(const mihevc_session *s) { if (s) { net = s->src.sr.net.get(); cnet = s->src.sr.cnet.get(); } }
    explicit operator bool() const { return net || cnet; }
    int scale() const { return cnet ? cnet->scale : net->scale; }
    int input_scale() const { return cnet ? 4 : net->scale; }      // what k_sr_input / k_sr_from_yuv are told: 2 unshuffles
    bool geometry_ok(int sw, int sh) const { return cnet ? sr_compact_geometry_ok(sw, sh) : sr_geometry_ok(net->scale, sw, sh); }
};
// What sr_prepare found for a source size: the network's tensor size tw x th, its output nw x nh, where the input tensor and the last layer's output lie in the
// arena, and the intermediate picture of the resized route
struct SrPlan { int tw, th, nw, nh, route; size_t x_off, out_off, moff[3]; int mstride[3], mpw, mph; };
// The arena of a source size, with the resized route (`route` 1) the intermediate picture and the tables.  An arena the device cannot hold: MIHEVC_ENOMEM,
// nothing launched, no planes taken, the session as it was
int sr_prepare(mihevc_session *s, const SrModelRef model, int src_width, int src_height, int route, SrPlan &pl)
{
    SourceFront::Sr &sr = s->src.sr;
    const SrCompactNet *const cnet = model.cnet;
    const int fct = model.input_scale() == 2 ? 2 : 1, tw = src_width / fct, th = src_height / fct, W = s->cfg.width, H = s->cfg.height;
    const int nw = model.scale() * src_width, nh = model.scale() * src_height, mw = route ? nw : 0, mh = route ? nh : 0;
    size_t off[SR_BUFS], coff[SRC_BUFS];
    const size_t bytes = cnet ? sr_compact_arena_layout(cnet->scale, tw, th, coff) : sr_arena_layout(tw, th, off), mbytes = sr_mid_layout(nw, nh, pl.moff, pl.mstride, pl.mpw, pl.mph);
    pl.tw = tw; pl.th = th; pl.nw = nw; pl.nh = nh; pl.route = route;
    pl.x_off = cnet ? coff[SRC_X] : off[SR_X]; pl.out_off = cnet ? coff[SRC_OUT] : off[SR_OUT];
    if (tw != sr.tw || th != sr.th || mw != sr.mw || mh != sr.mh || sr.arena.bytes() != bytes) {      // (the last: a model of the other kind or scale since)
        if (hipSetDevice(s->device) != hipSuccess) return MIHEVC_EDEVICE;
        HIPCK(s, hipStreamSynchronize(s->st_pre));      // launches still working in the arena of the last size
        sr.tw = sr.th = sr.mw = sr.mh = 0;
        sr.mid.reset();
        if (sr.arena.alloc(s->device, bytes, false) != hipSuccess) { (void)hipGetLastError(); return MIHEVC_ENOMEM; }
        if (route && sr.mid.alloc(s->device, mbytes, false) != hipSuccess) { (void)hipGetLastError(); sr.arena.reset(); return MIHEVC_ENOMEM; }
        sr.tw = tw; sr.th = th; sr.mw = mw; sr.mh = mh;
    }
    if (route)
        if (int e = sr.scale.ensure(s, nw, nh, [&](ScaleBlock &b) { return scale_block_build(nw, nh, W, H, SC_TH, SC_ROWS, b); })) return e;
    return MIHEVC_OK;
}
// The input tensor is written (or on its way on st_pre): the launches of the model, then k_ingest_rgb over the three half planes the last layer wrote: into the
// planes dp of coded size pw x ph at the session's depth, or into the intermediate picture that k_scale brings to the session's size
int sr_launch(mihevc_session *s, const SrModelRef model, const SrPlan &pl, RgbColour col, void *const *dp, const int *dstride, int pw, int ph)
{
    SourceFront::Sr &sr = s->src.sr;
    const int W = s->cfg.width, H = s->cfg.height, nw = pl.nw, nh = pl.nh;
    uint8_t *arena = sr.arena;
    if (model.cnet) HIPCK(s, launch_sr_compact_network(s->st_pre, *model.cnet, arena, (const uint16_t *)sr.wdev.get(), (const float *)(sr.wdev.get() + sr.bias_off), pl.tw, pl.th));
    else HIPCK(s, launch_sr_network(s->st_pre, *model.net, arena, (const uint16_t *)sr.wdev.get(), (const float *)(sr.wdev.get() + sr.bias_off), pl.tw, pl.th));
    const mihevc_rgb_format halves = {0, 0, 1, 2, 1, 0, 0, 0, {0, 0, 0, 0}};      // three planes of halves: R, G, B
    const uint16_t *o = (const uint16_t *)(arena + pl.out_off);
    if (!pl.route) {
        const IngestRgbArgs a = ingest_rgb_args(halves, col.matrix, col.full, o, o + (size_t)W * H, o + (size_t)2 * W * H, W, W, H, pw, ph, s->cfg.bit_depth, dp, dstride);
        HIPCK(s, launch_ingest_rgb(s->st_pre, a, 1, 2, s->is16));
        return MIHEVC_OK;
    }
    void *mid[3] = {sr.mid + pl.moff[0], sr.mid + pl.moff[1], sr.mid + pl.moff[2]};
    const IngestRgbArgs a = ingest_rgb_args(halves, col.matrix, col.full, o, o + (size_t)nw * nh, o + (size_t)2 * nw * nh, nw, nw, nh, pl.mpw, pl.mph, 10, mid, pl.mstride);
    HIPCK(s, launch_ingest_rgb(s->st_pre, a, 1, 2, true));
    const TapTables<ScaleBlock> &tab = sr.scale;
    const int32_t *first[4];
    const int16_t *coef[4];
    tap_pointers(tab.dev.get(), tab.host.first, first); tap_pointers(tab.dev.get(), tab.host.coef, coef);
    const ScaleArgs sa = scale_args(10, mid[0], mid[1], mid[2], pl.mstride[0], pl.mstride[1], nw, nh, W, H, pw, ph, s->cfg.bit_depth, dp, dstride, first, coef, tab.host.taps);
    HIPCK(s, launch_scale(s->st_pre, sa, true, s->is16));
    return MIHEVC_OK;
}
// A frame through the network (the arguments are checked, `route` is 0 or 1): sr_prepare; then input(pl, tensor) launches the kernel that writes the input
// tensor from the staged planes, and sr_launch follows, into the session's planes.  Everything on st_pre
template <typename Input>
int sr_frame(mihevc_session *s, const SrModelRef model, int src_width, int src_height, int route, RgbColour col, int flags, int64_t pts, SrcPlane *planes, int n, size_t es,
             Input &&input)
{
    SrPlan plan;
    if (int e = sr_prepare(s, model, src_width, src_height, route, plan)) return e;
    return convert_frame(s, SrcFlags::of(flags), pts, planes, n, es, [&](Src &dst, const SrcPlane *pl) -> int {
        if (int e = input(pl, (uint16_t *)(s->src.sr.arena.get() + plan.x_off))) return e;
        return sr_launch(s, model, plan, col, dst.p, dst.stride, s->w, s->h);
    });
}
// an R'G'B' source through the network: mihevc_send_frame_sr (fit false: the session is exactly scale x the source) and mihevc_send_frame_sr_fit
int send_sr_rgb(mihevc_session *s, const mihevc_rgb_format *fmt, int src_width, int src_height, const void *p0, const void *p1, const void *p2, int pitch, int64_t pts,
                int flags, bool fit)
{
    const void *p[3] = {p0, p1, p2};
    const bool fmt_ok = s && rgb_format_ok(fmt);
    const RgbColour col = rgb_colour(s, fmt, fmt_ok);
    const SrModelRef model(s);      // (false: no model)
    const bool geo_ok = fmt_ok && model && model.geometry_ok(src_width, src_height);
    const int route = geo_ok ? sr_route(s, model.scale() * src_width, model.scale() * src_height) : -1;
    const bool args_ok = geo_ok && rgb_matrix_ok(col.matrix) && (fit ? route >= 0 : route == 0) && rgb_planes_ok(*fmt, p, pitch, src_width);
    if (int e = refuse_source(s, args_ok, flags)) return e;
    const size_t es = (size_t)rgb_elem_size(*fmt);
    const int row = rgb_row_elems(*fmt, src_width);
    SrcPlane planes[3] = {{p[0], row, src_height, pitch}, {p[1], row, src_height, pitch}, {p[2], row, src_height, pitch}};
    return sr_frame(s, model, src_width, src_height, route, col, flags, pts, planes, rgb_planes(*fmt), es, [&](const SrcPlane *pl, uint16_t *x) -> int {
        const void *sp[3] = {pl[0].p, pl[1].p, pl[2].p};
        HIPCK(s, launch_sr_input(s->st_pre, sr_input_args(*fmt, model.input_scale(), src_width, src_height, sp, pl[0].pitch, x), fmt->sample, (int)es));
        return MIHEVC_OK;
    });
}

// ---- a chain of the filters (mihevc_set_source_chain, mihevc_send_frame_chain).  The stages are those of the single entries: ring_emit and fm_decide
// over the chain's own rings, the resize launches over the chain's own tables, each with the geometry csrc/chain_plan.h gives its stage and a ChainSink that hands
// the picture to the stage behind
using Chain = SourceFront::Chain;
constexpr int ST_F = SourceFront::ST_F, ST_D = SourceFront::ST_D, ST_R = SourceFront::ST_R, ST_I = SourceFront::ST_I, ST_END = SourceFront::ST_END;
inline int round8(int v) { return (v + 7) & ~7; }

// the first stage behind `from` that is on (from -1: the chain's first); ST_END: none
int chain_next(const ChainPlan &p, int from)
{
    const bool on[ST_END] = {p.field, p.denoise, p.resize, p.interp};
    for (int i = from + 1; i < ST_END; i++)
        if (on[i]) return i;
    return ST_END;
}
bool chain_decimates(const Chain &ch) { return ch.d.field == MIHEVC_CHAIN_FIELD_MATCH && ch.d.fieldmatch.decimate != 0; }
int chain_push(mihevc_session *s, int stage);
int chain_resize(mihevc_session *s, const void *const *in, const int *pitch);

// The sink of stage `from` of a chain.  The last stage writes a Src, which goes to the encoder as picture j at first_pts + j.  A stage in front of a ring stage
// writes that ring's next slot, a stage in front of the resize stage the hop picture; a decimating inverse telecine in front of either writes one of its
// kFmCycle hop pictures, which is copied into the slot, or resized, when its cycle lets it go.  Everything is on st_pre: a slot or hop picture is written again
// only behind the launches that read it.  Nothing here waits: mihevc_send_frame_chain does, once, at its end
struct ChainSink final : Sink {
    mihevc_session *s; Chain &ch; int next; bool hold;
    ChainSink(mihevc_session *s_, int from) : s(s_), ch(s_->src.chain), next(chain_next(s_->src.chain.plan, from)), hold(from == ST_F && next != ST_END && chain_decimates(s_->src.chain)) {}
    int take(Out &o) override
    {
        if (next == ST_END) return SrcSink(s, false).take(o);
        if (hold || next == ST_R) {      // the pictures a decimating inverse telecine holds come first, the one in front of the resize stage last
            const size_t held = chain_decimates(ch) && chain_next(ch.plan, ST_F) != ST_END ? (size_t)kFmCycle : 0;
            size_t i = hold ? 0 : held;
            while (hold && i < held && ch.hop_used[i]) i++;
            if (i >= (hold ? held : ch.hop.size())) return fail(s, "mihevc_send_frame_chain: no hop picture is free");
            ch.hop_used[i] = hold;
            o.hop = (int)i;
            for (int c = 0; c < 3; c++) { o.p[c] = ch.hop[i].p[c]; o.stride[c] = ch.hop[i].pitch[c]; }
            o.pw = round8(ch.plan.sw); o.ph = round8(ch.plan.sh);
            return MIHEVC_OK;
        }
        const Ring &r = ch.ring[next];
        for (int c = 0; c < 3; c++) { o.p[c] = r.p[r.n % 3][c]; o.stride[c] = r.pitch[c]; }
        o.pw = round8(r.w); o.ph = r.rows;
        return MIHEVC_OK;
    }
    int put(Out &&o, int64_t) override
    {
        if (next == ST_END) return finish_ingest(s, std::move(o.src), ch.first_pts + ch.pictures++, false);
        if (o.hop < 0) return chain_push(s, next);
        const SourceFront::Hop &h = ch.hop[(size_t)o.hop];
        ch.hop_used[(size_t)o.hop] = 0;
        if (next == ST_R) return chain_resize(s, h.p, h.pitch);
        const Ring &r = ch.ring[next];
        const size_t es = r.depth > 8 ? 2 : 1;
        for (int c = 0; c < 3; c++)
            HIPCK(s, hipMemcpy2DAsync(r.p[r.n % 3][c], r.pitch[c] * es, h.p[c], h.pitch[c] * es, (c ? r.w / 2 : r.w) * es, c ? r.h / 2 : r.h, hipMemcpyDeviceToDevice, s->st_pre));
        return chain_push(s, next);
    }
    void drop(Out &&o) override
    {
        if (o.hop >= 0) ch.hop_used[(size_t)o.hop] = 0;
        else s->free_src.push_back(std::move(o.src));
    }
};

// Slot n % 3 of the ring of `stage` holds a new frame (or will, in stream order): the picture(s) of the frame before it, as ingest_ring
int chain_push(mihevc_session *s, int stage)
{
    Chain &ch = s->src.chain;
    Ring &r = ch.ring[stage];
    const int64_t k = r.n;
    r.n = k + 1;
    if (r.kind == SourceFront::RING_FIELDMATCH) {
        std::lock_guard<std::mutex> l(s->m);
        s->src.fm.frames.push_back({{}, false});
    }
    ChainSink sink(s, stage);
    int e = MIHEVC_OK;
    if (k > 0) e = r.kind == SourceFront::RING_FIELDMATCH ? fm_decide(s, r, k - 1, true, sink) : ring_emit(s, r, k - 1, true, sink);
    r.pending = true;
    return e;
}

// The resize stage: a picture of the source's size and depth at `in` (the hop picture, or the staged planes of a chain that begins here) into the planes its sink
// names, at the session's size and depth, with the launch of mihevc_send_frame_scaled, mihevc_send_frame_upscaled or mihevc_send_frame_sr_yuv
int chain_resize(mihevc_session *s, const void *const *in, const int *pitch)
{
    Chain &ch = s->src.chain;
    const int W = s->cfg.width, H = s->cfg.height, sw = ch.plan.sw, sh = ch.plan.sh, sd = ch.plan.sd;
    ChainSink sink(s, ST_R);
    Out o;
    if (int e = sink.take(o)) return e;
    if (ch.d.resize == MIHEVC_CHAIN_RESIZE_SCALE) {
        const TapTables<ScaleBlock> &tab = ch.scale;
        const int32_t *first[4];
        const int16_t *coef[4];
        tap_pointers(tab.dev.get(), tab.host.first, first); tap_pointers(tab.dev.get(), tab.host.coef, coef);
        const ScaleArgs a = scale_args(sd, in[0], in[1], in[2], pitch[0], pitch[1], sw, sh, W, H, o.pw, o.ph, s->cfg.bit_depth, o.p, o.stride, first, coef, tab.host.taps);
        HIPCK(s, launch_scale(s->st_pre, a, sd > 8, s->is16));
    } else if (ch.d.resize == MIHEVC_CHAIN_RESIZE_UPSCALE) {
        const TapTables<UpscaleBlock> &tab = ch.upscale;
        const int32_t *first[4], *near[4];
        const int16_t *coef[4];
        tap_pointers(tab.dev.get(), tab.host.first, first); tap_pointers(tab.dev.get(), tab.host.near, near); tap_pointers(tab.dev.get(), tab.host.coef, coef);
        const UpscaleArgs a = upscale_args(ch.d.upscale, in[0], in[1], in[2], pitch[0], pitch[1], W, H, o.pw, o.ph, s->cfg.bit_depth, o.p, o.stride, first, near, coef);
        HIPCK(s, launch_upscale(s->st_pre, a, sd > 8, s->is16));
    } else {
        const SrModelRef model(s);
        SrPlan plan;
        if (int e = sr_prepare(s, model, sw, sh, sr_route(s, model.scale() * sw, model.scale() * sh), plan)) return e;      // (the entry has prepared this size: nothing is allocated here)
        HIPCK(s, launch_sr_from_yuv(s->st_pre, sr_yuv_args(ch.d.sr, model.input_scale(), in[0], in[1], in[2], pitch[0], pitch[1], (uint16_t *)(s->src.sr.arena.get() + plan.x_off)), sd > 8));
        if (int e = sr_launch(s, model, plan, RgbColour{s->cfg.matrix, s->cfg.full_range != 0}, o.p, o.stride, o.pw, o.ph)) return e;
    }
    return sink.put(std::move(o), 0);
}

// the session's model serves the chain's sr stage: there is one and the session's size is on one of its two routes
bool chain_sr_ok(const mihevc_session *s, const ChainPlan &p)
{
    const SrModelRef model(s);
    return model && model.geometry_ok(p.sw, p.sh) && sr_route(s, model.scale() * p.sw, model.scale() * p.sh) >= 0;
}

// Everything a chain allocates, at its first frame (DESIGN.md §6n states the bytes): the rings of the temporal stages, the hop picture(s), the blocks of the
// inverse telecine and of the interpolator, the tables of the resize stage or the network's arena.  A device that cannot hold them: MIHEVC_ENOMEM with nothing kept
int chain_setup(mihevc_session *s)
{
    Chain &ch = s->src.chain;
    const ChainPlan &p = ch.plan;
    SourceFront::Fm &fm = s->src.fm;
    const bool match = ch.d.field == MIHEVC_CHAIN_FIELD_MATCH;
    const int first = chain_next(p, -1);
    const bool holds = p.field && chain_next(p, ST_F) != ST_END && chain_decimates(ch);      // kFmCycle pictures held; a resize stage right behind reads them where they are
    const size_t n_hop = (holds ? (size_t)kFmCycle : 0) + (p.resize && (p.denoise || (p.field && !holds)) ? 1 : 0);
    // what can refuse the frame comes first (ensure keeps nothing of a size it could not build), so that no path leaves with blocks taken and the chain not ready
    const int W = p.dw, H = p.dh;
    if (ch.d.resize == MIHEVC_CHAIN_RESIZE_SCALE)
        if (int e = ch.scale.ensure(s, p.sw, p.sh, [&](ScaleBlock &b) { return scale_block_build(p.sw, p.sh, W, H, SC_TH, SC_ROWS, b); })) return e;
    if (ch.d.resize == MIHEVC_CHAIN_RESIZE_UPSCALE)
        if (int e = ch.upscale.ensure(s, p.sw, p.sh, [&](UpscaleBlock &b) { return upscale_block_build(p.sw, p.sh, W, H, UP_TH, UP_HALO, UP_ROWS, b); })) return e;
    if (match && !fm.ev) {
        fm.ev = Event(hipEventDisableTiming);
        if (!fm.ev) return fail(s, "mihevc_send_frame_chain: no event");
    }
    bool ok = true;
    // a ring a kernel writes has the rows of a coded picture; the chain's first ring is filled by copies
    if (p.field) ok = ok && ring_alloc(s, ch.ring[ST_F], match ? SourceFront::RING_FIELDMATCH : SourceFront::RING_DEINT, p.sw, p.sh, p.sd, p.sh) == hipSuccess;
    if (p.denoise) ok = ok && ring_alloc(s, ch.ring[ST_D], SourceFront::RING_DENOISE, p.sw, p.sh, p.sd, first == ST_D ? p.sh : round8(p.sh)) == hipSuccess;
    if (p.interp) ok = ok && ring_alloc(s, ch.ring[ST_I], SourceFront::RING_MCFI, p.dw, p.dh, p.dd, first == ST_I ? p.dh : round8(p.dh)) == hipSuccess;
    ch.hop.resize(n_hop);
    ch.hop_used.assign(n_hop, 0);
    for (auto &h : ch.hop) ok = ok && picture_alloc(s, h.mem, h.p, h.pitch, p.sw, round8(p.sh), p.sd > 8 ? 2 : 1) == hipSuccess;
    if (match) {
        const size_t bytes = ((size_t)fm_workgroups(p.sw, p.sh) + 1) * 8 * sizeof(unsigned long long);
        ok = ok && fm.dev.alloc(s->device, (bytes + 255) & ~(size_t)255, false) == hipSuccess && fm.host.alloc(s->device, 256, true) == hipSuccess;
    }
    if (p.interp) ok = ok && s->src.mcfi.dev.alloc(s->device, (mcfi_layout(p.dw, p.dh).bytes + 255) & ~(size_t)255, false) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        for (Ring &r : ch.ring)
            for (auto &m : r.mem) m.reset();
        ch.hop.clear();
        fm.dev.reset(); fm.host.reset(); s->src.mcfi.dev.reset();
        return MIHEVC_ENOMEM;
    }
    if (p.field && !match) { ch.ring[ST_F].deint_tff = ch.d.deint.tff; ch.ring[ST_F].deint_field_rate = ch.d.deint.field_rate; }
    if (match) { fm.mode = ch.d.fieldmatch; fm.open = true; }
    if (p.denoise) ch.ring[ST_D].denoise_pending = ch.d.denoise;
    if (p.interp) s->src.mcfi.pending = ch.d.interpolate;
    ch.ready = true;
    return MIHEVC_OK;
}

// mihevc_flush: the stages front to back.  A stage's last frame (its successor is itself) gives its picture(s) to the stage behind, whose own last frame
// follows; the interpolator's last frame gives its j = 0 picture
int chain_flush(mihevc_session *s)
{
    Chain &ch = s->src.chain;
    if (!ch.ready) return MIHEVC_OK;
    if (hipSetDevice(s->device) != hipSuccess) return MIHEVC_EDEVICE;
    for (int stage : {ST_F, ST_D, ST_I}) {
        Ring &r = ch.ring[stage];
        if (!r.pending) continue;
        ChainSink sink(s, stage);
        if (r.kind != SourceFront::RING_FIELDMATCH) {
            if (int e = ring_emit(s, r, r.n - 1, false, sink)) return e;
            continue;
        }
        if (int e = fm_decide(s, r, r.n - 1, false, sink)) return e;      // and what is left of an open cycle comes out whole
        if (int e = fm_release(s, -1, sink)) return e;
    }
    return MIHEVC_OK;
}

}  // namespace

template <typename Block> template <typename Build> int TapTables<Block>::ensure(mihevc_session *s, int sw_, int sh_, Build build)
{
    if (sw == sw_ && sh == sh_) return MIHEVC_OK;
    Block blk;
    if (!build(blk)) return MIHEVC_EINVAL;
    if (hipSetDevice(s->device) != hipSuccess) return MIHEVC_EDEVICE;
    sw = sh = 0;
    HIPCK(s, hipStreamSynchronize(s->st_pre));      // a launch still reading the tables of the size before
    HIPCK(s, dev.alloc(s->device, blk.bytes.size(), false));
    host = std::move(blk);
    HIPCK(s, hipMemcpyAsync(dev, host.bytes.data(), host.bytes.size(), hipMemcpyHostToDevice, s->st_pre));
    sw = sw_; sh = sh_;
    return MIHEVC_OK;
}

int source_flush(mihevc_session *s)
{
    if (s->src.chain.set) return chain_flush(s);
    Ring &r = s->src.ring;
    if (!r.pending) return MIHEVC_OK;
    if (hipSetDevice(s->device) != hipSuccess) return MIHEVC_EDEVICE;
    SrcSink sink(s, false);
    if (r.kind != SourceFront::RING_FIELDMATCH) return ring_emit(s, r, r.n - 1, false, sink);
    if (int e = fm_decide(s, r, r.n - 1, false, sink)) return e;      // and what is left of an open cycle comes out whole
    return fm_release(s, -1, sink);
}

extern "C" {

int mihevc_send_frame(mihevc_session *s, const void *y, const void *u, const void *v, int pitch_y, int pitch_c, int64_t pts)
{
    return ingest(s, y, u, v, pitch_y, pitch_c, pts, SrcFlags{false, false});
}
int mihevc_send_frame_async(mihevc_session *s, const void *y, const void *u, const void *v, int pitch_y, int pitch_c, int64_t pts)
{
    return ingest(s, y, u, v, pitch_y, pitch_c, pts, SrcFlags{false, true});
}
int mihevc_send_frame_device(mihevc_session *s, const void *y, const void *u, const void *v, int pitch_y, int pitch_c, int64_t pts)
{
    return ingest(s, y, u, v, pitch_y, pitch_c, pts, SrcFlags{true, false});
}
int mihevc_send_frames_device(mihevc_session *s, int n, const void *const *y, const void *const *u, const void *const *v, int pitch_y, int pitch_c, int64_t first_pts)
{
    if (!s || n < 0 || (n && (!y || !u || !v))) return MIHEVC_EINVAL;
    for (int i = 0; i < n; i++)
        if (int e = ingest(s, y[i], u[i], v[i], pitch_y, pitch_c, first_pts + i, SrcFlags{true, false})) return e;
    return MIHEVC_OK;
}
// A source in another layout (mihevc_send_frame_fmt): k_ingest writes the session's own planes, margin included, from the caller's device planes or from their
// copies in the staging set
int mihevc_send_frame_fmt(mihevc_session *s, const mihevc_src_format *fmt, const void *y, const void *u, const void *v, int pitch_y, int pitch_c, int64_t pts, int flags)
{
    const bool args_ok = s && src_format_ok(fmt) && y && u && (v || fmt->semi_planar) && pitch_y >= s->cfg.width && pitch_c >= src_chroma_row(*fmt, s->cfg.width);
    if (int e = refuse_source(s, args_ok, flags)) return e;
    // the session's own layout: the existing route, copy and margin fill.  Device planes are copied too, never borrowed: this entry point lets the caller have
    // them back after mihevc_sync_uploads, whatever the format
    if (fmt->chroma == 420 && !fmt->semi_planar && fmt->bit_depth == s->cfg.bit_depth && !fmt->msb_aligned)
        return ingest(s, y, u, v, pitch_y, pitch_c, pts, SrcFlags::of(flags), false);
    const size_t es = fmt->bit_depth > 8 ? 2 : 1;
    const int W = s->cfg.width, H = s->cfg.height, crow = src_chroma_row(*fmt, W), crows = src_chroma_rows(*fmt, H);
    SrcPlane planes[3] = {{y, W, H, pitch_y}, {u, crow, crows, pitch_c}, {v, crow, crows, pitch_c}};
    return convert_frame(s, SrcFlags::of(flags), pts, planes, fmt->semi_planar ? 2 : 3, es, [&](Src &dst, const SrcPlane *pl) -> int {
        const IngestArgs a = ingest_args(*fmt, pl[0].p, pl[1].p, pl[2].p, pl[0].pitch, pl[1].pitch, W, H, s->w, s->h, s->cfg.bit_depth, dst.p, dst.stride);
        HIPCK(s, launch_ingest(s->st_pre, a, es == 2, s->is16));
        return MIHEVC_OK;
    });
}
// An RGB source (mihevc_send_frame_rgb; matrix and range resolved): as mihevc_send_frame_fmt, with k_ingest_rgb
int mihevc_send_frame_rgb(mihevc_session *s, const mihevc_rgb_format *fmt, const void *p0, const void *p1, const void *p2, int pitch, int64_t pts, int flags)
{
    const void *p[3] = {p0, p1, p2};
    const bool fmt_ok = s && rgb_format_ok(fmt);
    const RgbColour col = rgb_colour(s, fmt, fmt_ok);
    if (int e = refuse_source(s, fmt_ok && rgb_matrix_ok(col.matrix) && rgb_planes_ok(*fmt, p, pitch, s->cfg.width), flags)) return e;
    const size_t es = (size_t)rgb_elem_size(*fmt);
    const int W = s->cfg.width, H = s->cfg.height, row = rgb_row_elems(*fmt, W);
    SrcPlane planes[3] = {{p[0], row, H, pitch}, {p[1], row, H, pitch}, {p[2], row, H, pitch}};
    return convert_frame(s, SrcFlags::of(flags), pts, planes, rgb_planes(*fmt), es, [&](Src &dst, const SrcPlane *pl) -> int {
        const IngestRgbArgs a = ingest_rgb_args(*fmt, col.matrix, col.full, pl[0].p, pl[1].p, pl[2].p, pl[0].pitch, W, H, s->w, s->h, s->cfg.bit_depth, dst.p, dst.stride);
        HIPCK(s, launch_ingest_rgb(s->st_pre, a, fmt->sample, (int)es, s->is16));
        return MIHEVC_OK;
    });
}
int mihevc_set_lut3d(mihevc_session *s, int n, const uint16_t *table)
{
    if (!s || s->cfg.slice_count > 1 || (table && !lut3d_n_ok(n))) return MIHEVC_EINVAL;
    if (s->failed) return s->fail_code;
    SourceFront::Lut &lut = s->src.lut;
    if (!table) { lut.n = 0; return MIHEVC_OK; }
    if (hipSetDevice(s->device) != hipSuccess) return MIHEVC_EDEVICE;
    const size_t cap = ((size_t)LUT_MAX_N * LUT_MAX_N * LUT_MAX_N * LUT_ENTRY_BYTES + 255) & ~(size_t)255;      // the largest table: every block is allocated once
    if (!lut.dev) HIPCK(s, lut.dev.alloc(s->device, cap, false));
    uint8_t *block;
    HIPCK(s, lut.host.acquire(s->device, cap, block));      // the copy of the table before the last one
    lut3d_pack(n, table, (uint16_t *)block);
    HIPCK(s, lut.host.commit(lut.dev, (size_t)n * n * n * LUT_ENTRY_BYTES, s->st_pre));
    lut.n = n;
    return MIHEVC_OK;
}
// A source through the colour table (mihevc_send_frame_lut3d; a table is set): as mihevc_send_frame_fmt, with k_lut3d
int mihevc_send_frame_lut3d(mihevc_session *s, const mihevc_lut3d_src *src, const void *y, const void *u, const void *v, int pitch_y, int pitch_c, int64_t pts, int flags)
{
    const bool args_ok = s && lut3d_src_ok(src) && s->src.lut.n && rgb_matrix_ok(s->cfg.matrix) && lut3d_planes_ok(*src, y, u, v, pitch_y, pitch_c, s->cfg.width);
    if (int e = refuse_source(s, args_ok, flags)) return e;
    const size_t es = src->bit_depth > 8 ? 2 : 1;
    const int W = s->cfg.width, H = s->cfg.height;
    SrcPlane planes[3] = {{y, W, H, pitch_y}, {u, W / 2, H / 2, pitch_c}, {v, W / 2, H / 2, pitch_c}};
    return convert_frame(s, SrcFlags::of(flags), pts, planes, 3, es, [&](Src &dst, const SrcPlane *pl) -> int {
        const Lut3dArgs a = lut3d_args(*src, s->src.lut.n, s->src.lut.dev.get(), pl[0].p, pl[1].p, pl[2].p, pl[0].pitch, pl[1].pitch, W, H, s->w, s->h, s->cfg.bit_depth,
                                       s->cfg.matrix, s->cfg.full_range != 0, dst.p, dst.stride);
        HIPCK(s, launch_lut3d(s->st_pre, a, es == 2, s->is16));
        return MIHEVC_OK;
    });
}
// A source of another size (mihevc_send_frame_scaled): k_scale writes the session's own planes, margin included, from the caller's device planes or from their
// copies in the staging set.  The tables of a new source size are built before the first device call
int mihevc_send_frame_scaled(mihevc_session *s, const mihevc_scale_src *src, const void *y, const void *u, const void *v, int pitch_y, int pitch_c, int64_t pts, int flags)
{
    const bool args_ok = s && scale_src_ok(src) && y && u && v && scale_geometry_ok(src->width, src->height, s->cfg.width, s->cfg.height) &&
                         pitch_y >= src->width && pitch_c >= src->width / 2;
    if (int e = refuse_source(s, args_ok, flags)) return e;
    const int W = s->cfg.width, H = s->cfg.height;
    TapTables<ScaleBlock> &tab = s->src.scale;
    if (int e = tab.ensure(s, src->width, src->height, [&](ScaleBlock &b) { return scale_block_build(src->width, src->height, W, H, SC_TH, SC_ROWS, b); })) return e;
    const size_t es = src->bit_depth > 8 ? 2 : 1;
    SrcPlane planes[3] = {{y, src->width, src->height, pitch_y}, {u, src->width / 2, src->height / 2, pitch_c}, {v, src->width / 2, src->height / 2, pitch_c}};
    return convert_frame(s, SrcFlags::of(flags), pts, planes, 3, es, [&](Src &dst, const SrcPlane *pl) -> int {
        const int32_t *first[4];
        const int16_t *coef[4];
        tap_pointers(tab.dev.get(), tab.host.first, first); tap_pointers(tab.dev.get(), tab.host.coef, coef);
        const ScaleArgs a = scale_args(src->bit_depth, pl[0].p, pl[1].p, pl[2].p, pl[0].pitch, pl[1].pitch, src->width, src->height, W, H, s->w, s->h, s->cfg.bit_depth, dst.p, dst.stride,
                                       first, coef, tab.host.taps);
        HIPCK(s, launch_scale(s->st_pre, a, es == 2, s->is16));
        return MIHEVC_OK;
    });
}
// A smaller source (mihevc_send_frame_upscaled): as mihevc_send_frame_scaled, with k_upscale and the session's own block of its tables
int mihevc_send_frame_upscaled(mihevc_session *s, const mihevc_upscale_src *src, const void *y, const void *u, const void *v, int pitch_y, int pitch_c, int64_t pts, int flags)
{
    const bool args_ok = s && upscale_src_ok(src) && y && u && v && upscale_geometry_ok(src->width, src->height, s->cfg.width, s->cfg.height) &&
                         pitch_y >= src->width && pitch_c >= src->width / 2;
    if (int e = refuse_source(s, args_ok, flags)) return e;
    const int W = s->cfg.width, H = s->cfg.height;
    TapTables<UpscaleBlock> &tab = s->src.upscale;
    if (int e = tab.ensure(s, src->width, src->height, [&](UpscaleBlock &b) { return upscale_block_build(src->width, src->height, W, H, UP_TH, UP_HALO, UP_ROWS, b); })) return e;
    const size_t es = src->bit_depth > 8 ? 2 : 1;
    SrcPlane planes[3] = {{y, src->width, src->height, pitch_y}, {u, src->width / 2, src->height / 2, pitch_c}, {v, src->width / 2, src->height / 2, pitch_c}};
    return convert_frame(s, SrcFlags::of(flags), pts, planes, 3, es, [&](Src &dst, const SrcPlane *pl) -> int {
        const int32_t *first[4], *near[4];
        const int16_t *coef[4];
        tap_pointers(tab.dev.get(), tab.host.first, first); tap_pointers(tab.dev.get(), tab.host.near, near); tap_pointers(tab.dev.get(), tab.host.coef, coef);
        const UpscaleArgs a = upscale_args(*src, pl[0].p, pl[1].p, pl[2].p, pl[0].pitch, pl[1].pitch, W, H, s->w, s->h, s->cfg.bit_depth, dst.p, dst.stride, first, near, coef);
        HIPCK(s, launch_upscale(s->st_pre, a, es == 2, s->is16));
        return MIHEVC_OK;
    });
}
// The packed weights and the fp32 parameters of a model of either kind on their way to the session's device block: on st_pre, behind every launch that reads the
// model before.  MIHEVC_ENOMEM leaves the session without a model
static int sr_upload_model(mihevc_session *s, const std::vector<uint16_t> &wpk, const std::vector<float> &par)
{
    SourceFront::Sr &sr = s->src.sr;
    if (hipSetDevice(s->device) != hipSuccess) return MIHEVC_EDEVICE;
    const size_t wbytes = (wpk.size() * sizeof(uint16_t) + 255) & ~(size_t)255, total = wbytes + par.size() * sizeof(float);
    if (sr.wdev.bytes() != total) {      // a model of another size: new blocks, on the device and (in acquire) on the host
        HIPCK(s, hipStreamSynchronize(s->st_pre));      // launches still reading the block of the last model
        sr.net.reset();
        sr.cnet.reset();
        if (sr.wdev.alloc(s->device, total, false) != hipSuccess) { (void)hipGetLastError(); return MIHEVC_ENOMEM; }
    }
    uint8_t *block;
    HIPCK(s, sr.whost.acquire(s->device, total, block));      // the copy of the model before the last one
    memcpy(block, wpk.data(), wpk.size() * sizeof(uint16_t));
    memcpy(block + wbytes, par.data(), par.size() * sizeof(float));
    HIPCK(s, sr.whost.commit(sr.wdev, total, s->st_pre));
    sr.bias_off = wbytes;
    return MIHEVC_OK;
}
int mihevc_set_sr_model(mihevc_session *s, const mihevc_sr_model *model, const float *weights, size_t count)
{
    if (!s || s->cfg.slice_count > 1) return MIHEVC_EINVAL;
    SourceFront::Sr &sr = s->src.sr;
    if (!model) {
        if (s->failed) return s->fail_code;
        sr.net.reset();
        sr.cnet.reset();
        return MIHEVC_OK;
    }
    if (!sr_model_ok(model) || !weights || count != sr_net_count(model->scale, model->blocks)) return MIHEVC_EINVAL;
    if (s->failed) return s->fail_code;
    std::unique_ptr<SrNet> net(new SrNet);
    if (!sr_net_build(model->scale, model->blocks, weights, count, *net)) return MIHEVC_EINVAL;
    if (int e = sr_upload_model(s, net->wpk, net->bias)) return e;
    net->wpk = std::vector<uint16_t>();      // the launches need the shapes and the list, not the host copy of the weights
    sr.cnet.reset();
    sr.net = std::move(net);
    return MIHEVC_OK;
}
int mihevc_set_sr_compact(mihevc_session *s, const mihevc_sr_compact *model, const float *weights, size_t count)
{
    if (!s || s->cfg.slice_count > 1) return MIHEVC_EINVAL;
    if (!sr_compact_ok(model) || !weights || count != sr_compact_count(model->scale, model->convs)) return MIHEVC_EINVAL;
    if (s->failed) return s->fail_code;
    std::unique_ptr<SrCompactNet> net(new SrCompactNet);
    if (!sr_compact_build(model->scale, model->convs, weights, count, *net)) return MIHEVC_EINVAL;
    if (int e = sr_upload_model(s, net->wpk, net->par)) return e;
    net->wpk = std::vector<uint16_t>();
    net->par = std::vector<float>();
    s->src.sr.net.reset();
    s->src.sr.cnet = std::move(net);
    return MIHEVC_OK;
}
// A smaller R'G'B' source through the network (mihevc_send_frame_sr; a model is set): k_sr_input in front of sr_frame
int mihevc_send_frame_sr(mihevc_session *s, const mihevc_rgb_format *fmt, int src_width, int src_height, const void *p0, const void *p1, const void *p2, int pitch,
                         int64_t pts, int flags)
{
    return send_sr_rgb(s, fmt, src_width, src_height, p0, p1, p2, pitch, pts, flags, false);
}
int mihevc_send_frame_sr_fit(mihevc_session *s, const mihevc_rgb_format *fmt, int src_width, int src_height, const void *p0, const void *p1, const void *p2, int pitch,
                             int64_t pts, int flags)
{
    return send_sr_rgb(s, fmt, src_width, src_height, p0, p1, p2, pitch, pts, flags, true);
}
// A planar 4:2:0 Y'CbCr source through the network (mihevc_send_frame_sr_yuv): k_sr_from_yuv in front of sr_frame; the output side is the session's matrix and range
int mihevc_send_frame_sr_yuv(mihevc_session *s, const mihevc_sr_yuv *src, const void *y, const void *u, const void *v, int pitch_y, int pitch_c, int64_t pts, int flags)
{
    const SrModelRef model(s);
    const bool src_ok = s && model && sr_yuv_src_ok(src);
    const int route = src_ok ? sr_route(s, model.scale() * src->width, model.scale() * src->height) : -1;
    const bool args_ok = src_ok && route >= 0 && rgb_matrix_ok(s->cfg.matrix) && sr_yuv_planes_ok(*src, y, u, v, pitch_y, pitch_c);
    if (int e = refuse_source(s, args_ok, flags)) return e;
    const size_t es = src->bit_depth > 8 ? 2 : 1;
    const int sw = src->width, sh = src->height;
    SrcPlane planes[3] = {{y, sw, sh, pitch_y}, {u, sw / 2, sh / 2, pitch_c}, {v, sw / 2, sh / 2, pitch_c}};
    return sr_frame(s, model, sw, sh, route, RgbColour{s->cfg.matrix, s->cfg.full_range != 0}, flags, pts, planes, 3, es, [&](const SrcPlane *pl, uint16_t *x) -> int {
        HIPCK(s, launch_sr_from_yuv(s->st_pre, sr_yuv_args(*src, model.input_scale(), pl[0].p, pl[1].p, pl[2].p, pl[0].pitch, pl[1].pitch, x), es == 2));
        return MIHEVC_OK;
    });
}
int mihevc_send_frame_deint(mihevc_session *s, const mihevc_deint *d, const void *y, const void *u, const void *v, int pitch_y, int pitch_c, int64_t pts, int flags)
{
    const bool args_ok = s && deint_mode_ok(d) && y && u && v &&
                         (s->src.ring.kind != SourceFront::RING_DEINT || (d->tff == s->src.ring.deint_tff && d->field_rate == s->src.ring.deint_field_rate)) &&
                         deint_geometry_ok(s->cfg.width, s->cfg.height) && pitch_y >= s->cfg.width && pitch_c >= s->cfg.width / 2;
    if (int e = refuse_source(s, args_ok, flags, SourceFront::RING_DEINT)) return e;
    if (s->src.ring.kind == SourceFront::RING_NONE) { s->src.ring.deint_tff = d->tff; s->src.ring.deint_field_rate = d->field_rate; }
    return ingest_ring(s, SourceFront::RING_DEINT, y, u, v, pitch_y, pitch_c, pts, SrcFlags::of(flags));
}
int mihevc_send_frame_denoise(mihevc_session *s, const mihevc_denoise *d, const void *y, const void *u, const void *v, int pitch_y, int pitch_c, int64_t pts, int flags)
{
    const bool args_ok = s && denoise_strength_ok(d) && y && u && v && denoise_geometry_ok(s->cfg.width, s->cfg.height) && pitch_y >= s->cfg.width &&
                         pitch_c >= s->cfg.width / 2;
    if (int e = refuse_source(s, args_ok, flags, SourceFront::RING_DENOISE)) return e;
    const int e = ingest_ring(s, SourceFront::RING_DENOISE, y, u, v, pitch_y, pitch_c, pts, SrcFlags::of(flags));
    s->src.ring.denoise_pending = *d;      // (the picture of the frame before has been launched with its own)
    return e;
}
int mihevc_send_frame_interpolate(mihevc_session *s, const mihevc_interpolate *d, const void *y, const void *u, const void *v, int pitch_y, int pitch_c, int64_t pts, int flags)
{
    const bool args_ok = s && mcfi_mode_ok(d) && y && u && v &&
                         (s->src.ring.kind != SourceFront::RING_MCFI || (d->factor == s->src.mcfi.pending.factor && d->mode == s->src.mcfi.pending.mode)) &&
                         mcfi_geometry_ok(s->cfg.width, s->cfg.height) && pitch_y >= s->cfg.width && pitch_c >= s->cfg.width / 2;
    if (int e = refuse_source(s, args_ok, flags, SourceFront::RING_MCFI)) return e;
    if (hipSetDevice(s->device) != hipSuccess) return MIHEVC_EDEVICE;
    if (!s->src.mcfi.dev) {
        HIPCK(s, s->src.mcfi.dev.alloc(s->device, (mcfi_layout(s->cfg.width, s->cfg.height).bytes + 255) & ~(size_t)255, false));
        s->src.mcfi.pending = *d;
    }
    const int e = ingest_ring(s, SourceFront::RING_MCFI, y, u, v, pitch_y, pitch_c, pts, SrcFlags::of(flags));
    s->src.mcfi.pending.scene_threshold = d->scene_threshold;      // (the pictures of the frame before have been launched with its own)
    return e;
}
int mihevc_send_frame_fieldmatch(mihevc_session *s, const mihevc_fieldmatch *d, const void *y, const void *u, const void *v, int pitch_y, int pitch_c, int64_t pts, int flags)
{
    const bool args_ok = s && fieldmatch_mode_ok(d) && y && u && v &&
                         (!s->src.fm.open || (d->tff == s->src.fm.mode.tff && d->decimate == s->src.fm.mode.decimate && d->deint == s->src.fm.mode.deint)) &&
                         deint_geometry_ok(s->cfg.width, s->cfg.height) && pitch_y >= s->cfg.width && pitch_c >= s->cfg.width / 2;
    if (int e = refuse_source(s, args_ok, flags, SourceFront::RING_FIELDMATCH)) return e;
    if (hipSetDevice(s->device) != hipSuccess) return MIHEVC_EDEVICE;
    SourceFront::Fm &fm = s->src.fm;
    if (!fm.open) {
        const size_t bytes = ((size_t)fm_workgroups(s->cfg.width, s->cfg.height) + 1) * 8 * sizeof(unsigned long long);
        if (!fm.ev) fm.ev = Event(hipEventDisableTiming);
        if (!fm.ev) return fail(s, "mihevc_send_frame_fieldmatch: no event");
        HIPCK(s, fm.dev.alloc(s->device, (bytes + 255) & ~(size_t)255, false));
        HIPCK(s, fm.host.alloc(s->device, 256, true));
        fm.mode = *d; fm.first_pts = pts; fm.open = true;
    }
    {
        std::lock_guard<std::mutex> l(s->m);
        fm.frames.push_back({{}, false});
    }
    return ingest_ring(s, SourceFront::RING_FIELDMATCH, y, u, v, pitch_y, pitch_c, pts, SrcFlags::of(flags));
}
int mihevc_set_source_chain(mihevc_session *s, const mihevc_chain *chain)
{
    if (!s || s->cfg.slice_count > 1) return MIHEVC_EINVAL;
    const SrModelRef model(s);
    if (!chain_check(chain, s->cfg.width, s->cfg.height, s->cfg.bit_depth, s->cfg.matrix, model ? model.scale() : 0)) return MIHEVC_EINVAL;
    if (s->failed) return s->fail_code;
    Chain &ch = s->src.chain;
    if (ch.set || s->flushed || s->frames_in > 0 || s->src.ring.n > 0 || s->src.fm.open || !s->pending.empty()) return MIHEVC_ESTATE;
    const ChainPlan plan = chain_plan(*chain, s->cfg.width, s->cfg.height, s->cfg.bit_depth);
    if (chain->resize == MIHEVC_CHAIN_RESIZE_SR && !chain_sr_ok(s, plan)) return MIHEVC_EINVAL;
    ch.d = *chain;
    ch.plan = plan;
    ch.set = true;
    return MIHEVC_OK;
}
// A frame through the session's chain (mihevc_send_frame_chain): into the first stage's ring, as ingest_ring, or through the staging set into the resize stage;
// the stages hand their pictures on themselves (ChainSink)
int mihevc_send_frame_chain(mihevc_session *s, const void *y, const void *u, const void *v, int pitch_y, int pitch_c, int64_t pts, int flags)
{
    if (!s) return MIHEVC_EINVAL;
    Chain &ch = s->src.chain;
    const bool args_ok = y && u && v && (!ch.set || (pitch_y >= ch.plan.sw && pitch_c >= ch.plan.sw / 2 && (ch.frames == 0 || pts > ch.last_pts)));
    if (!args_ok || (flags & ~(MIHEVC_SRC_DEVICE | MIHEVC_SRC_ASYNC))) return MIHEVC_EINVAL;
    if (s->failed) return s->fail_code;
    if (!ch.set || s->flushed) return MIHEVC_ESTATE;
    if (ch.d.resize == MIHEVC_CHAIN_RESIZE_SR && !chain_sr_ok(s, ch.plan)) return MIHEVC_EINVAL;      // (the model was dropped or replaced since)
    if (hipSetDevice(s->device) != hipSuccess) return MIHEVC_EDEVICE;
    if (!ch.ready)
        if (int e = chain_setup(s)) return e;
    if (ch.d.resize == MIHEVC_CHAIN_RESIZE_SR) {      // the arena of this size: MIHEVC_ENOMEM before anything is launched
        const SrModelRef model(s);
        SrPlan plan;
        if (int e = sr_prepare(s, model, ch.plan.sw, ch.plan.sh, sr_route(s, model.scale() * ch.plan.sw, model.scale() * ch.plan.sh), plan)) return e;
    }
    const SrcFlags fl = SrcFlags::of(flags);
    const ChainPlan &p = ch.plan;
    const size_t es = p.sd > 8 ? 2 : 1;
    const int first = chain_next(p, -1);
    if (ch.frames == 0) ch.first_pts = pts;
    ch.frames++;
    ch.last_pts = pts;
    int e;
    if (first == ST_R) {
        SrcPlane planes[3] = {{y, p.sw, p.sh, pitch_y}, {u, p.sw / 2, p.sh / 2, pitch_c}, {v, p.sw / 2, p.sh / 2, pitch_c}};
        if (int e2 = stage_planes(s, planes, 3, es, fl.device)) return e2;
        const void *in[3] = {planes[0].p, planes[1].p, planes[2].p};
        const int pitch[3] = {planes[0].pitch, planes[1].pitch, planes[2].pitch};
        e = chain_resize(s, in, pitch);
    } else {
        const Ring &r = ch.ring[first];
        const void *in[3] = {y, u, v};
        for (int c = 0; c < 3; c++)
            HIPCK(s, hipMemcpy2DAsync(r.p[r.n % 3][c], r.pitch[c] * es, in[c], (c ? pitch_c : pitch_y) * es, (c ? r.w / 2 : r.w) * es, c ? r.h / 2 : r.h,
                                      fl.device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s->st_pre));
        e = chain_push(s, first);
    }
    if (e) return e;
    if (fl.wait()) HIPCK(s, hipStreamSynchronize(s->st_pre));      // once, behind whatever the stages launched: the caller's planes are free
    else s->up_pending = true;
    return MIHEVC_OK;
}
int mihevc_get_fieldmatch_info(mihevc_session *s, int64_t frame, mihevc_fm_frame *out)
{
    if (!s || !out) return MIHEVC_EINVAL;
    std::lock_guard<std::mutex> l(s->m);
    if (frame < 0 || (size_t)frame >= s->src.fm.frames.size()) return MIHEVC_EINVAL;
    if (!s->src.fm.frames[(size_t)frame].decided) return MIHEVC_EAGAIN;
    *out = s->src.fm.frames[(size_t)frame].info;
    return MIHEVC_OK;
}

}  // extern "C"
