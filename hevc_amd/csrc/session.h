// hevc_amd/csrc/session.h — the session as its two translation units see it (private: not installed, not part of include/).  session.cpp is the encoder proper:
// chunks, rate control, halo exchange, publishing.  source.cpp is the source front end: every mihevc_send_frame* entry, down to enqueue_source.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <condition_variable>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "bitstream.h"
#include "chain_plan.h"
#include "device.h"
#include "gop_plan.h"
#include "host_pool.h"
#include "ratectl.h"
#include "scale_taps.h"
#include "slice_group.h"

using namespace mihevc;

constexpr int kRing = 12;     // symbol slots per lane (capacity): slot 0 holds the IDR picture, the rest rotate over the P steps.
                              // A session uses s->ring of them: 8 up to 1080p-class levels, 12 from level 5 (2160p+), where the CABAC of one
                              // picture (12 ms at 2160p, 45 ms at 4320p) outlasts five device steps when few GOP lanes are busy
constexpr int kGroups = 2;        // lane groups of a chunk's P/B steps: two launch sequences on two streams (encode_chunk)

struct Packet {
    std::vector<uint8_t> data;
    int64_t pts = 0, dts = 0;
    bool key = false, ready = false;
    std::string error;      // the host coder refused the picture's levels (sign data hiding parity): mihevc_receive_packet fails with MIHEVC_EINVAL here
};

// a session's scratch buffer from the process-wide cache (grow()): device memory, optionally with a pinned host twin of the same size
struct CachedBuf { CachedBlock<uint8_t> d, h; };

// a source picture of the current chunk (device).  borrowed: the caller's device planes, not copied (mem is empty)
struct Src { CachedBlock<uint8_t> mem[3]; void *p[3]; int stride[3]; int64_t pts; bool borrowed; };
// where a kernel of the front end writes a picture, as a sink names it (source.cpp): the planes of `src`, or (a chain) of hop picture `hop` or of a
// ring's slot; pw x ph: the coded size the kernel fills
struct Out { Src src; int hop = -1; void *p[3] = {}; int stride[3] = {}; int pw = 0, ph = 0; };

// The coefficient tables (csrc/scale_taps.h: Block is ScaleBlock or UpscaleBlock) of the last source size of a resampling entry, built and uploaded once per
// size; the host copy lives as long as the device block it is copied from on st_pre
template <typename Block> struct TapTables {
    CachedBlock<uint8_t> dev; Block host; int sw = 0, sh = 0;
    // the tables of a sw_ x sh_ source are on the device, or on their way on st_pre.  build(Block &): the tables of a new size; it runs before the first device
    // call, and false is MIHEVC_EINVAL with the tables of the size before still in place.  tap_pointers(dev, host.first, ..) finds a table in the device block
    template <typename Build> int ensure(mihevc_session *s, int sw_, int sh_, Build build);
};

// The state of the source front end (source.cpp), by concern
struct SourceFront {
    // mihevc_send_frame_fmt, host planes: the raw planes in the SOURCE layout on their way to k_ingest.  Copy and conversion of a picture are neighbours on st_pre,
    // so the next picture's copy comes behind this picture's kernel in stream order: one set serves every picture (a set per pending picture would be 12 MB
    // each for a 1080p 4:4:4 16-bit source).  It grows when a larger format arrives (st_pre is synchronised first) and goes back with the session
    CachedBlock<uint8_t> stage;
    // mihevc_send_frame_scaled: the four coefficient tables (csrc/scale_taps.h) of the last source size, built and uploaded once per size; the host copy lives as
    // long as the device block it is copied from on st_pre
    TapTables<ScaleBlock> scale;
    // mihevc_send_frame_upscaled: its own block of tables (scale_taps.h, upscale_block_build) of the last source size, kept as the downscaler's is
    TapTables<UpscaleBlock> upscale;
    // mihevc_set_sr_model, mihevc_send_frame_sr: the network as csrc/sr_net.h packs it.  net is the host copy (launch list and shapes; null: no
    // model), wdev the packed weights and then the biases in one device block, copied on st_pre from one of two pinned blocks taken in turn as the LUT's are (PinnedPair, host_pool.h), so a
    // new model follows every launch that reads the old one in stream order; a model of another size waits for st_pre first and takes a new block.  arena:
    // the activations of the last source size (sr_net_bytes), allocated at the first frame of a size
    // mihevc_send_frame_sr_yuv, mihevc_send_frame_sr_fit into a session smaller than the network's output: mid is the intermediate 4:2:0 picture at 10 bit of
    // mw x mh = the network's output size (0: none; its planes and strides: sr_mid_layout), taken and let go with the arena; scale: the tables that bring it to
    // the session's size, an instance of its own so that mihevc_send_frame_scaled keeps its tables
    // mihevc_set_sr_compact: cnet is the compact network as csrc/sr_compact_net.h packs it.  At most one of net and cnet is set; both kinds share
    // wdev (packed weights, then the fp32 parameters at bias_off), whost, arena and mid, so a session that sets no compact model allocates and launches nothing more
    struct Sr {
        std::unique_ptr<SrNet> net; std::unique_ptr<SrCompactNet> cnet; CachedBlock<uint8_t> wdev, arena, mid; PinnedPair whost; size_t bias_off = 0; int tw = 0, th = 0, mw = 0, mh = 0;
        TapTables<ScaleBlock> scale;
    } sr;
    // mihevc_set_lut3d, mihevc_send_frame_lut3d: the packed table of n points per axis (0: none) in one device block of the largest size,
    // so a new table of any size overwrites the old one in stream order on st_pre, behind every k_lut3d launch that reads it and in front of the next.  It is
    // copied from one of two pinned blocks, taken in turn; a block is written again only behind the event of the copy that read it, two tables back
    struct Lut { CachedBlock<uint8_t> dev; PinnedPair host; int n = 0; } lut;
    // mihevc_send_frame_deint, mihevc_send_frame_denoise, mihevc_send_frame_fieldmatch, mihevc_send_frame_interpolate: a ring of three source-size pictures (display size, rows that begin 16-byte aligned), allocated at the
    // first call; frame k lies in slot k % 3.  Copies and k_deint / k_denoise launches are neighbours on st_pre, so a slot is overwritten in stream order behind
    // the last launch that read it.  kind: the entry that filled the ring first (a pending frame keeps every other entry out until flush, so it is the only
    // one); n: frames taken; pending: the last of them has not produced its picture(s) yet (the next frame or mihevc_flush does that)
    // The ring is a value: w x h at `depth` is what ITS pictures are (the session's ring: the session's display size and depth; a chain's rings: their
    // stage's), rows the rows of a slot (a slot a kernel writes is rounded up to 8 as a coded picture is: the stores come in runs)
    enum { RING_NONE = 0, RING_DEINT, RING_DENOISE, RING_FIELDMATCH, RING_MCFI };
    struct Ring {
        CachedBlock<uint8_t> mem[3]; void *p[3][3] = {}; int pitch[3] = {};
        int w = 0, h = 0, depth = 0, rows = 0;
        int64_t n = 0, pts = 0; int kind = RING_NONE; bool pending = false;
        int deint_tff = 0, deint_field_rate = 0;
        mihevc_denoise denoise_pending = {};      // the strengths of the pending frame
    } ring;
    // mihevc_send_frame_interpolate: pending: factor and mode of the session's first interpolated frame, the scene threshold of the pending
    // one; dev: vectors, SAD0(0), the parts of D and D (mcfi_layout), written and read in stream order on st_pre
    struct Mcfi { mihevc_interpolate pending = {}; CachedBlock<uint8_t> dev; } mcfi;
    // mihevc_send_frame_fieldmatch: the frames go through the same ring.  open: from the first fieldmatch frame until flush no other entry
    // sends a frame.  dev: the partials of k_fm_metrics and the eight folded numbers behind them; host: their pinned copy, valid behind ev.  frames:
    // what was decided, by frame (decided: mihevc_get_fieldmatch_info may hand it out; under the session's `m`).  held: decimate: the filled pictures of the open
    // cycle with their frames' numbers; pictures: pictures handed on so far
    struct Fm {
        bool open = false; mihevc_fieldmatch mode = {}; CachedBlock<uint8_t> dev, host; Event ev;
        struct Frame { mihevc_fm_frame info; bool decided; };
        std::vector<Frame> frames; std::vector<std::pair<Out, int64_t>> held;
        int64_t pictures = 0, first_pts = 0;
    } fm;
    // mihevc_set_source_chain, mihevc_send_frame_chain: d is the descriptor, plan what csrc/chain_plan.h says of it.  ring[F], ring[D], ring[I]:
    // one ring per temporal stage that is on, at its stage's size and depth; a stage's kernel writes the next ring's slot.  hop: pictures at the source's size and
    // depth: kFmCycle when a decimating inverse telecine is not the last stage (it holds them where the entry holds Srcs; hop_used: which are held), then one
    // in front of the resize stage when a kernel writes it (the held pictures are resized where they are).  The inverse telecine and the interpolator keep their state where their entries do (fm, mcfi).  ready: the blocks are allocated
    // (the first frame); pictures: handed to the session so far, the j-th at first_pts + j; last_pts: of the last frame
    enum { ST_F = 0, ST_D, ST_R, ST_I, ST_END };
    struct Hop { CachedBlock<uint8_t> mem; void *p[3] = {}; int pitch[3] = {}; };
    struct Chain {
        bool set = false, ready = false; mihevc_chain d = {}; ChainPlan plan = {};
        Ring ring[ST_END];
        std::vector<Hop> hop; std::vector<char> hop_used;
        TapTables<ScaleBlock> scale; TapTables<UpscaleBlock> upscale;
        int64_t frames = 0, pictures = 0, first_pts = 0, last_pts = 0;
    } chain;
};

struct mihevc_session {
    mihevc_config cfg;
    int device = 0;
    int w = 0, h = 0, ctus_w = 0, ctus_h = 0, n_ctu = 0;      // coded size
    TileGrid tiles;                                            // IDR pictures (PPS 1); 1x1 when cfg.intra_tiles == 0
    TileGrid ptiles;                                           // P pictures (PPS 0, cfg.p_tiles); 1x1 when off
    int keyint = 90, lanes = 4, me_range = 16, qp_p = 22, qp_i = 19;
    bool is16 = false, keep_recon = false, flushed = false, flushing = false;
    std::atomic<bool> failed{false};     // sticky (fail()); mihevc_abort sets it from another thread
    int fail_code = MIHEVC_EDEVICE;      // what calls return once `failed` is set: MIHEVC_EINVAL when the host coder refused a picture
    std::string err;                     // written under `m` (mihevc_abort may run on another thread)
    CachedStream st_compute, st_copy, st_pre;      // st_pre: the chunk's pre-search, beside the IDR step; then the P/B steps of lane group 1
    int lane_groups = kGroups;        // launch sequences the P/B steps of a chunk run as (MIHEVC_LANE_GROUPS, read at mihevc_open: 1 = one sequence on the compute stream)
    // uploads of host frames (mihevc_send_frame / _async) go through st_pre (idle outside a chunk's IDR step; a FOURTH stream per session made two of them share a
    // hardware queue: the copy stream's SSE pass and symbol copies then queued behind the compute stream's kernels, +10 ms of bubbles per 300-frame clip); the
    // chunk's first launch waits for ev_up
    Event ev_up{hipEventDisableTiming};
    bool up_pending = false;
    // source pictures of the current chunk (device), in display order
    std::vector<Src> pending;
    std::vector<Src> free_src;
    SourceFront src;                  // everything in front of `pending` (source.cpp)
    // per lane
    // The vector moves a lane's handles when it grows; the blocks they own stay where they are, so the raw pointers in argument blocks, jobs and BandPub stay valid
    struct Lane {
        CachedBlock<uint8_t> rec_mem[3][3]; void *rec_p[3][3] = {}; int rec_stride[3] = {};       // padded final reconstructions: the anchors ping-pong between 0 and 1; 2 = B pictures (cfg.bframes; never a reference)
        CachedBlock<uint8_t> work_mem[3]; void *work_p[3] = {}; int work_stride[3] = {};           // pre-deblock / deblocked picture (unpadded)
        CachedBlock<int32_t> me, me1;      // integer-search tables (me1: list 1 of B pictures)
        CachedBlock<IpInfo> ip;            // per CTU: inter pass -> intra second pass of P pictures
        CachedBlock<IntraPlan> plan;       // per CTU: k_intra_plan -> k_intra_diag (IDR pictures)
        CachedBlock<uint8_t> sym_dev[kRing], sym_host[kRing];
        CachedBlock<uint8_t> md5_host[kRing];      // cfg.pic_hash 1: the final picture (coded size, Y U V without gaps), pinned, per ring slot
    };
    std::vector<Lane> lane;
    CachedBuf args;                   // argument blocks of a whole chunk (device + pinned staging)
    CachedBlock<unsigned long long> est_host;      // step 0 under rate control: the lanes' rate estimates (MAX_LANES pinned words; session.cpp queue_estimates), taken at the first use
    // by (lane group, ring slot); step 0 (all lanes, one launch) uses group 0's slot 0.  compute: the step's pictures are final; copy: its symbols are on the
    // host; jobs_open: its CABAC jobs still running (under `m`)
    struct Slot { Event compute{hipEventDisableTiming}, copy{hipEventDisableTiming}; int jobs_open = 0; } slot[kGroups][kRing];
    Event ev_join{hipEventDisableTiming};     // behind the last step of lane group 1 (st_pre): the compute stream waits for it at the end of the chunk
    Event t_begin{hipEventDefault}, t_end{hipEventDefault};      // a chunk's device time (stats.device_ms)
    std::vector<Event> ev_pool;        // profile_stages: start/stop pairs
    struct Mark { int stage, pictures; size_t ev; };
    std::vector<Mark> marks;
    // host side
    ThreadPool *pool = nullptr;
    std::mutex m;
    std::condition_variable cv;
    int ring = 8;                 // slots in use (<= kRing)
    int host_threads = 2;         // CABAC worker threads this session asked the process-wide pool for
    std::map<int64_t, Packet> packets;     // by output index
    int64_t next_out = 0, frames_in = 0, frames_done = 0;
    std::vector<uint8_t> headers, cur_packet;
    std::vector<std::vector<uint8_t>> cur_batch;      // what the last mihevc_receive_packets handed out (cur_packet: the last mihevc_receive_packet); either call releases them
    std::map<int64_t, std::vector<uint16_t>> recon;   // keep_recon: final pictures by index (Y,U,V concatenated)
    mihevc_stats stats{};
    RateControl rc;                           // rate control (csrc/ratectl.h)
    CachedBuf probe;                          // cfg.bframes = -1: the probe's argument blocks
    int64_t pts_step = 1, first_pts = 0;      // pts distance of the first two frames: with B pictures dts = (pts of the frame at the packet's place in decoding order) - pts_step
    GopState gop;                             // what the GOP planner carries from chunk to chunk (csrc/gop_plan.h)
    CachedBuf low;                                   // per chunk: 1/4-size SOURCE pictures of every picture, then the search centres of every picture (pre-search)
    Event ev_pre{hipEventDisableTiming}, ev_args{hipEventDisableTiming};  // the chunk's centres are ready (st_pre) / the IDR step's k_intra_plan is through (compute stream: the argument blocks are on the device too)
    CachedBuf scene;                                 // per chunk: picture pointers / pitches in, difference sums out (k_scene_diff)
    std::vector<FrameRec> frames;             // by output index
    struct Quality { unsigned long long sse[3]; long long ssim[3]; bool known; };
    std::vector<Quality> quality;             // by output index (display order), written when the picture's symbols have landed (publish_picture)
    std::atomic<long long> entropy_ns{0};
    bool events_ok() const      // the events the session is constructed with (an Event that could not be created is empty)
    {
        bool ok = ev_up && ev_join && t_begin && t_end && ev_pre && ev_args;
        for (auto &g : slot) for (auto &sl : g) ok = ok && sl.compute && sl.copy;
        return ok;
    }
    // ---- one slice of a picture whose slices exchange rows (cfg.slice_halo; csrc/slice_group.h)
    std::shared_ptr<SliceGroup> group;
    int band = 0, n_bands = 1;
    int band_h[kMaxBands] = {0};              // coded heights of all bands
    long long gstep = 0;                      // steps since the session was opened: the same in every band of the group
    Event ev_x1[2], ev_x2[2];
    CachedBlock<uint8_t> x1_export[2];
    size_t x1_part_bytes = 0, x1_lane_bytes = 0;
    CachedBuf jobs;                           // row-copy job tables of a chunk (device + pinned staging)
    std::vector<int> peers_enabled;
    // ---- decoded picture hash (cfg.pic_hash)
    CachedBlock<uint32_t> hash_part;          // 2 / 3: segment partials of k_pic_hash, MAX_LANES pictures (device)
    // ---- per-picture SSIM (cfg.ssim)
    CachedBlock<long long> ssim_part;         // region partials of k_ssim, MAX_LANES pictures (device)
    long long ssim_total[3] = {0, 0, 0};      // sum of Q over every window of every published picture: an integer, so mihevc_stats.ssim_* does not depend on the
                                              // order the CABAC jobs finish in (2 M windows of a 4320p picture x 2^32 x 500 000 pictures fit 63 bits)
};

// ---- what both sides call (session.cpp, but for source_flush: source.cpp, the front end's part of mihevc_flush)
int fail(mihevc_session *s, std::string msg);
#define HIPCK(s, expr)                                                                    \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess) return fail((s), std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)
inline size_t esize(const mihevc_session *s) { return s->is16 ? 2 : 1; }
int alloc_planes(mihevc_session *s, CachedBlock<uint8_t> mem[3], void *p[3], int stride[3], int padded);
int enqueue_source(mihevc_session *s, Src &&src, int64_t pts);
int source_flush(mihevc_session *s);
