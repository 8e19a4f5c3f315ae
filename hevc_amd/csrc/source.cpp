// hevc_amd/csrc/source.cpp — the source front end of a session: every mihevc_send_frame* entry, from the caller's picture in any layout through
// any filter to enqueue_source, all on st_pre.  It meets the encoder proper (session.cpp) at take_src, at finish_ingest / enqueue_source and at source_flush; its
// state is mihevc_session::src (session.h).  A converting entry is written against convert_frame: it describes the caller's planes and hands over a callable that
// builds the kernel's arguments and launches it; the device, the set of planes, the staging of host planes and the hand-over to the session are the frame's.
#include <cstring>
#include <utility>

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
    if (s->flushed || s->src.ring.pending || s->src.fm.open) return MIHEVC_ESTATE;      // (a deinterlaced or denoised frame waits for its successor: no other picture may come between; fieldmatch cycles are not interleaved)
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

// Frame k of the ring produces its picture(s): P = frame k - 1 (the first frame: itself), C = frame k, N = frame k + 1 (has_next; the last frame: itself)
struct RingFrames { void *const *P, *const *C, *const *N; };
RingFrames ring_take(mihevc_session *s, int64_t k, bool has_next)
{
    SourceFront::Ring &r = s->src.ring;
    r.pending = false;
    return {r.p[(k > 0 ? k - 1 : k) % 3], r.p[k % 3], r.p[(has_next ? k + 1 : k) % 3]};
}

// The picture(s) of frame k of the ring (mihevc_send_frame_deint, mihevc_send_frame_denoise): P, C, N as ring_take.  k_deint / k_denoise / k_mcfi_render write the
// session's own planes, margin included, out of the ring.  Deinterlacing: frame-rate mode keeps the first field's rows, field-rate mode follows with the second field's
// picture at pts + 1.  Denoising: one picture, with the strengths frame k came with.  Interpolation (mihevc_send_frame_interpolate): the vectors of the pair (C, N),
// then `factor` pictures at pts + j; the last frame: its own picture only
int ring_emit(mihevc_session *s, int64_t k, bool has_next, bool wait)
{
    SourceFront::Ring &r = s->src.ring;
    const auto [P, C, N] = ring_take(s, k, has_next);
    const bool denoise = r.kind == SourceFront::RING_DENOISE;
    if (r.kind == SourceFront::RING_MCFI) {      // the pictures between C and N; the last frame: itself (picture 0 of a blend with any N)
        mihevc_interpolate m = s->src.mcfi.pending;
        if (!has_next) m.mode = 1;
        const int W = s->cfg.width, H = s->cfg.height;
        const McfiLayout l = mcfi_layout(W, H);
        uint8_t *const blk = s->src.mcfi.dev.get();
        if (m.mode == 0) {
            const McfiSearchArgs a = mcfi_search_args(s->cfg.bit_depth, C[0], N[0], r.pitch[0], W, H, blk);
            HIPCK(s, launch_mcfi_vectors(s->st_pre, a, mcfi_field_args(a, blk), s->is16));
        }
        for (int j = 0; j < (has_next ? m.factor : 1); j++) {
            Src src;
            if (int e = take_src(s, src)) return e;
            const McfiRenderArgs a = mcfi_render_args(m, j, s->cfg.bit_depth, C, N, r.pitch[0], r.pitch[1], W, H, s->w, s->h, (const int16_t *)(blk + l.v),
                                                      (const unsigned long long *)(blk + l.dsum), src.p, src.stride);
            HIPCK(s, launch_mcfi_render(s->st_pre, a, s->is16));
            if (int e = finish_ingest(s, std::move(src), r.pts + j, wait)) return e;
        }
        return MIHEVC_OK;
    }
    const int first = r.deint_tff ? 0 : 1;
    for (int f = 0; f <= (denoise ? 0 : r.deint_field_rate); f++) {
        Src src;
        if (int e = take_src(s, src)) return e;
        if (denoise) {
            const DenoiseArgs a = denoise_args(r.denoise_pending, s->cfg.bit_depth, P, C, N, r.pitch[0], r.pitch[1], s->cfg.width, s->cfg.height, s->w, s->h, src.p, src.stride);
            HIPCK(s, launch_denoise(s->st_pre, a, s->is16));
        } else {
            const DeintArgs a = deint_args(s->cfg.bit_depth, P, C, N, r.pitch[0], r.pitch[1], s->cfg.width, s->cfg.height, s->w, s->h, f ? 1 - first : first, f, src.p, src.stride);
            HIPCK(s, launch_deint(s->st_pre, a, s->is16));
        }
        if (int e = finish_ingest(s, std::move(src), r.pts + f, wait)) return e;
    }
    return MIHEVC_OK;
}

// decimate: the held pictures go on in order, all but the one at `drop` (-1: a partial cycle comes out whole), whose planes go back to free_src
int fm_release(mihevc_session *s, int drop, bool wait)
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
        if (dropped || e) { s->free_src.push_back(std::move(held[i].first)); continue; }
        e = finish_ingest(s, std::move(held[i].first), fm.first_pts + fm.pictures++, wait);
    }
    return e;
}

// Frame k of the ring is decided (mihevc_send_frame_fieldmatch): P, C, N as ring_take.  The metrics of the frame are taken on st_pre and copied to
// pinned memory behind fm.ev; the host waits for that event only, plans (csrc/fieldmatch_plan.h) and launches the weave, or the deinterlacer, into a Src.
// Without decimate the picture goes on with its frame's pts; with it the picture is held until its cycle's fifth frame is decided
int fm_decide(mihevc_session *s, int64_t k, bool has_next, bool wait)
{
    SourceFront::Ring &r = s->src.ring;
    SourceFront::Fm &fm = s->src.fm;
    const auto [P, C, N] = ring_take(s, k, has_next);
    const int W = s->cfg.width, H = s->cfg.height, keep = fm.mode.tff ? 0 : 1;
    const size_t nwg = (size_t)fm_workgroups(W, H);
    unsigned long long *const part = (unsigned long long *)fm.dev.get(), *const host = (unsigned long long *)fm.host.get();
    HIPCK(s, launch_fm_metrics(s->st_pre, fm_args(s->cfg.bit_depth, P[0], C[0], N[0], r.pitch[0], W, H, keep, part), part + nwg * 8, s->is16));
    HIPCK(s, hipMemcpyAsync(host, part + nwg * 8, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s->st_pre));
    HIPCK(s, hipEventRecord(fm.ev, s->st_pre));
    HIPCK(s, hipEventSynchronize(fm.ev));
    FmMetrics m = fm_metrics_of(host);
    if (k == 0) fm_first_frame(m);
    const int match = fm_match(m);
    const bool fallback = fm_falls_back(m, match, fm.mode.deint != 0);
    Src src;
    if (int e = take_src(s, src)) return e;
    if (fallback) {
        const DeintArgs a = deint_args(s->cfg.bit_depth, P, C, N, r.pitch[0], r.pitch[1], W, H, s->w, s->h, keep, 0, src.p, src.stride);
        HIPCK(s, launch_deint(s->st_pre, a, s->is16));
    } else {
        void *const *X = match == 0 ? C : match == 1 ? P : N;
        const DeintArgs a = deint_args(s->cfg.bit_depth, X, C, X, r.pitch[0], r.pitch[1], W, H, s->w, s->h, keep, 0, src.p, src.stride);
        HIPCK(s, launch_fm_weave(s->st_pre, a, s->is16));
    }
    mihevc_fm_frame info = {};
    for (int i = 0; i < 3; i++) { info.comb_sum[i] = m.comb_sum[i]; info.comb_block[i] = m.comb_block[i]; }
    info.dup_sum = m.dup_sum; info.dup_block = m.dup_block; info.match = match; info.deinterlaced = fallback; info.dropped = 0;
    info.picture = fm.mode.decimate ? -1 : fm.pictures;
    {
        std::lock_guard<std::mutex> l(s->m);
        fm.frames[(size_t)k] = {info, !fm.mode.decimate};
    }
    if (!fm.mode.decimate) { fm.pictures++; return finish_ingest(s, std::move(src), r.pts, wait); }
    fm.held.emplace_back(std::move(src), k);
    if ((int)fm.held.size() < kFmCycle) return MIHEVC_OK;
    FmMetrics cycle[kFmCycle] = {};
    for (int i = 0; i < kFmCycle; i++) {
        const mihevc_fm_frame &f = fm.frames[(size_t)fm.held[(size_t)i].second].info;
        cycle[i].dup_sum = f.dup_sum; cycle[i].dup_block = f.dup_block;
    }
    return fm_release(s, fm_drop(cycle), wait);
}

// A frame of kind `kind` (mihevc_send_frame_deint, mihevc_send_frame_denoise; the arguments are checked): into its slot of the ring, then the picture(s) of the frame
// before it.  Returns with ring.pts still that of the frame before: the caller sets what belongs to the new frame
int ingest_ring(mihevc_session *s, int kind, const void *y, const void *u, const void *v, int pitch_y, int pitch_c, int64_t pts, SrcFlags fl)
{
    if (hipSetDevice(s->device) != hipSuccess) return MIHEVC_EDEVICE;
    SourceFront::Ring &r = s->src.ring;
    const size_t es = esize(s);
    const int W = s->cfg.width, H = s->cfg.height;
    if (!r.mem[0]) {
        r.pitch[0] = (W + 15) & ~15; r.pitch[1] = r.pitch[2] = (W / 2 + 15) & ~15;
        const size_t by = ((size_t)r.pitch[0] * H * es + 255) & ~(size_t)255, bc = ((size_t)r.pitch[1] * (H / 2) * es + 255) & ~(size_t)255;
        for (int k = 0; k < 3; k++) {
            HIPCK(s, r.mem[k].alloc(s->device, by + 2 * bc, false));
            r.p[k][0] = r.mem[k]; r.p[k][1] = r.mem[k] + by; r.p[k][2] = r.mem[k] + by + bc;
        }
        r.kind = kind;
    }
    const int64_t k = r.n;
    const void *in[3] = {y, u, v};
    for (int c = 0; c < 3; c++)
        HIPCK(s, hipMemcpy2DAsync(r.p[k % 3][c], r.pitch[c] * es, in[c], (c ? pitch_c : pitch_y) * es, (c ? W / 2 : W) * es, c ? H / 2 : H,
                                  fl.device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s->st_pre));
    r.n = k + 1;
    const bool wait = fl.wait();
    int e = MIHEVC_OK;
    if (k > 0) e = kind == SourceFront::RING_FIELDMATCH ? fm_decide(s, k - 1, true, wait) : ring_emit(s, k - 1, true, wait);      // (ring.pts and denoise_pending are still those of frame k - 1)
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
    return s->flushed || (s->src.ring.pending && s->src.ring.kind != kind) ? MIHEVC_ESTATE : MIHEVC_OK;
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
// A frame through the network (the arguments are checked, `route` is 0 or 1): the arena of the size, with the resized route the intermediate picture and the
// tables; then input(pl, tensor) launches the kernel that writes the input tensor from the staged planes, the launches of the model follow, and k_ingest_rgb
// over the three half planes the last layer wrote: into the session's planes, or into the intermediate picture that k_scale brings to the session's size.
// Everything on st_pre.  An arena the device cannot hold: MIHEVC_ENOMEM, nothing launched, no planes taken, the session as it was
template <typename Input>
int sr_frame(mihevc_session *s, const SrModelRef model, int src_width, int src_height, int route, RgbColour col, int flags, int64_t pts, SrcPlane *planes, int n, size_t es,
             Input &&input)
{
    SourceFront::Sr &sr = s->src.sr;
    const SrNet *const net = model.net;
    const SrCompactNet *const cnet = model.cnet;
    const int fct = model.input_scale() == 2 ? 2 : 1, tw = src_width / fct, th = src_height / fct, W = s->cfg.width, H = s->cfg.height;
    const int nw = model.scale() * src_width, nh = model.scale() * src_height, mw = route ? nw : 0, mh = route ? nh : 0;
    size_t off[SR_BUFS], coff[SRC_BUFS], moff[3];
    int mstride[3], mpw, mph;
    const size_t bytes = cnet ? sr_compact_arena_layout(cnet->scale, tw, th, coff) : sr_arena_layout(tw, th, off), mbytes = sr_mid_layout(nw, nh, moff, mstride, mpw, mph);
    const size_t x_off = cnet ? coff[SRC_X] : off[SR_X], out_off = cnet ? coff[SRC_OUT] : off[SR_OUT];
    if (tw != sr.tw || th != sr.th || mw != sr.mw || mh != sr.mh || sr.arena.bytes() != bytes) {      // (the last: a model of the other kind or scale since)
        if (hipSetDevice(s->device) != hipSuccess) return MIHEVC_EDEVICE;
        HIPCK(s, hipStreamSynchronize(s->st_pre));      // launches still working in the arena of the last size
        sr.tw = sr.th = sr.mw = sr.mh = 0;
        sr.mid.reset();
        if (sr.arena.alloc(s->device, bytes, false) != hipSuccess) { (void)hipGetLastError(); return MIHEVC_ENOMEM; }
        if (route && sr.mid.alloc(s->device, mbytes, false) != hipSuccess) { (void)hipGetLastError(); sr.arena.reset(); return MIHEVC_ENOMEM; }
        sr.tw = tw; sr.th = th; sr.mw = mw; sr.mh = mh;
    }
    TapTables<ScaleBlock> &tab = sr.scale;
    if (route)
        if (int e = tab.ensure(s, nw, nh, [&](ScaleBlock &b) { return scale_block_build(nw, nh, W, H, SC_TH, SC_ROWS, b); })) return e;
    return convert_frame(s, SrcFlags::of(flags), pts, planes, n, es, [&](Src &dst, const SrcPlane *pl) -> int {
        uint8_t *arena = sr.arena;
        if (int e = input(pl, (uint16_t *)(arena + x_off))) return e;
        if (cnet) HIPCK(s, launch_sr_compact_network(s->st_pre, *cnet, arena, (const uint16_t *)sr.wdev.get(), (const float *)(sr.wdev.get() + sr.bias_off), tw, th));
        else HIPCK(s, launch_sr_network(s->st_pre, *net, arena, (const uint16_t *)sr.wdev.get(), (const float *)(sr.wdev.get() + sr.bias_off), tw, th));
        const mihevc_rgb_format halves = {0, 0, 1, 2, 1, 0, 0, 0, {0, 0, 0, 0}};      // three planes of halves: R, G, B
        const uint16_t *o = (const uint16_t *)(arena + out_off);
        if (!route) {
            const IngestRgbArgs a = ingest_rgb_args(halves, col.matrix, col.full, o, o + (size_t)W * H, o + (size_t)2 * W * H, W, W, H, s->w, s->h, s->cfg.bit_depth, dst.p, dst.stride);
            HIPCK(s, launch_ingest_rgb(s->st_pre, a, 1, 2, s->is16));
            return MIHEVC_OK;
        }
        void *mid[3] = {sr.mid + moff[0], sr.mid + moff[1], sr.mid + moff[2]};
        const IngestRgbArgs a = ingest_rgb_args(halves, col.matrix, col.full, o, o + (size_t)nw * nh, o + (size_t)2 * nw * nh, nw, nw, nh, mpw, mph, 10, mid, mstride);
        HIPCK(s, launch_ingest_rgb(s->st_pre, a, 1, 2, true));
        const int32_t *first[4];
        const int16_t *coef[4];
        tap_pointers(tab.dev.get(), tab.host.first, first); tap_pointers(tab.dev.get(), tab.host.coef, coef);
        const ScaleArgs sa = scale_args(10, mid[0], mid[1], mid[2], mstride[0], mstride[1], nw, nh, W, H, s->w, s->h, s->cfg.bit_depth, dst.p, dst.stride, first, coef, tab.host.taps);
        HIPCK(s, launch_scale(s->st_pre, sa, true, s->is16));
        return MIHEVC_OK;
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
    const SourceFront::Ring &r = s->src.ring;
    if (!r.pending) return MIHEVC_OK;
    if (hipSetDevice(s->device) != hipSuccess) return MIHEVC_EDEVICE;
    if (r.kind != SourceFront::RING_FIELDMATCH) return ring_emit(s, r.n - 1, false, false);
    if (int e = fm_decide(s, r.n - 1, false, false)) return e;      // and what is left of an open cycle comes out whole
    return fm_release(s, -1, false);
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
