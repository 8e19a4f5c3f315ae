/* include/mihevc.h — C ABI of the MI355X-native HEVC encode path (libmihevc.so).
 *
 * This is the drop-in boundary.  The reference has no FFI: its encode step is the child process
 * `ffmpeg -c:v libx265|hevc_nvenc` spawned by run_ffmpeg (reference core/transcoder.py:497-535) with the operating
 * point built by build_ffmpeg_params (core/transcoder.py:357-412).  The entry points below are what a binding for
 * that step would call instead; hevc_amd/encoder.py is that binding (ctypes), INTEGRATION.md shows the stub a
 * maintainer of the reference would add.
 *
 * Conventions: plain C types only; every int-returning function returns 0 (MIHEVC_OK) or a negative mihevc_err;
 * nothing throws or aborts; distinct sessions may be used from distinct threads concurrently (the reference calls
 * convert_video from N QThreads, gui/mainwindow.py:289-301); one session is driven by one thread at a time.
 * ctypes releases the GIL during calls, which that threading model relies on.
 */
#ifndef MIHEVC_H
#define MIHEVC_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIHEVC_ABI_VERSION 6

typedef enum {
    MIHEVC_OK = 0,
    MIHEVC_EAGAIN = -1,     /* receive_packet: nothing ready yet (send more frames or flush) */
    MIHEVC_EOF = -2,        /* receive_packet after flush: stream complete */
    MIHEVC_EINVAL = -3,     /* bad argument / unsupported configuration */
    MIHEVC_ENODEV = -4,     /* no gfx950 device (or HIP runtime unusable) */
    MIHEVC_ENOMEM = -5,
    MIHEVC_EDEVICE = -6,    /* HIP call failed; see mihevc_last_error */
    MIHEVC_ESTATE = -7      /* call sequence error (e.g. send after flush) */
} mihevc_err;

/* Encoder operating point.  Field-for-field this is what the reference passes to libx265 through
 * `-x265-params` (core/transcoder.py:398-411) plus the HDR10 set of core/utils.py:58-69. */
typedef struct mihevc_config {
    int32_t width, height;            /* display size; coded size is rounded up to a multiple of 8 + conformance window */
    int32_t fps_num, fps_den;         /* VUI/VPS timing */
    int32_t bit_depth;                /* 8 (Main) or 10 (Main10) */
    int32_t level_idc;                /* general_level_idc = 30 * level  (x265 level-idc) */
    int32_t tier;                     /* 0 main, 1 high                  (x265 tier) */
    int32_t crf;                      /* constant-quality target         (x265 crf); frame QP is derived from it */
    int32_t qp;                       /* >= 0: force this QP for P frames (I frames qp-3); -1: derive from crf */
    int32_t vbv_maxrate_kbps;         /* x265 vbv-maxrate; 0 = unconstrained */
    int32_t vbv_bufsize_kbits;        /* x265 vbv-bufsize */
    int32_t keyint, min_keyint;       /* closed GOP length (IDR period)  (x265 keyint / min-keyint) */
    int32_t colour_primaries, transfer, matrix;   /* VUI code points: 1/1/1 bt709, 9/16/9 HDR10 (x265 colorprim/transfer/colormatrix) */
    int32_t full_range;               /* 0: `-color_range tv` (core/transcoder.py:490) */
    int32_t chroma_loc;               /* -1: not signalled; 0..5 chroma_sample_loc_type (x265 chromaloc) */
    int32_t aud;                      /* emit access unit delimiters     (x265 aud) */
    int32_t repeat_headers;           /* VPS/SPS/PPS before every IDR    (x265 repeat-headers); the first IDR always has them */
    int32_t hdr10;                    /* emit SEI 137 + 144              (x265 hdr10 / master-display / max-cll) */
    uint16_t md_primaries[3][2];      /* G,B,R (x,y) in 0.00002 units */
    uint16_t md_white[2];
    uint32_t md_max_lum, md_min_lum;  /* 0.0001 cd/m2 */
    uint16_t max_cll, max_fall;
    int32_t me_range;                 /* integer search +-range (<= 64); 0 = default */
    int32_t gops_in_flight;           /* closed GOPs encoded in lock-step on the device; 0 = default */
    int32_t host_threads;             /* CABAC worker threads; 0 = default */
    int32_t sao;                      /* 1 (default -1 -> 1) enable SAO */
    int32_t profile_stages;           /* 1: bracket every stage launch with HIP events on the compute stream (mihevc_stats.stage_ms); 2: only the
                                       * dominant stage (inter_ctu) — ~180 instead of ~1250 events per 300 pictures, which cost 5 % of the throughput */
    int32_t intra_tiles;              /* 1 (default): IDR pictures use the largest uniform tile grid the level allows (PPS 1), which
                                       * cuts the intra CTU wavefront from W+2H to w+2h CTUs of one tile; 0: one tile */
    int32_t intra_nxn;                /* 1: 8x8 intra CUs are also tried as four 4x4 PUs (part_mode NxN, DST-VII 4x4 luma TUs).  Default 0:
                                       * on the bench clip the trial costs 2 ms per IDR picture (-15 % fps) and wins in 0.4 % of the CUs */
    int32_t intra_in_p;               /* 1: P pictures run an intra second pass over CTUs the reference predicts badly (two independent-set
                                       * rounds, so isolated CTUs and the first CTUs of a blob).  Default 0: each round costs one
                                       * serial CTU-program latency, 0.12 ms per 1080p picture, and the bench clip gains nothing from it */
    int32_t hrd;                      /* 1: HRD parameters in the VUI + buffering-period SEI at every IDR + picture-timing SEI per picture
                                       * (x265 hrd=1, part of the reference's HDR10 set, core/utils.py:66); needs vbv_maxrate/bufsize */
    int32_t pre_search;               /* 1 (default): search centres from a +-14 full search on the 1/4-size pictures, so the +-me_range
                                       * integer search follows motion up to +-56 samples; 0: centres at zero.  A session searches the 1/4-size SOURCE
                                       * picture against the SOURCE picture before it, for a whole chunk at once (beside the IDR step) */
    int32_t rdo_zero;                 /* 1 (default): inter TUs whose levels cost more (lambda x bits) than the distortion they remove are
                                       * coded as all-zero (whole 300-picture bench clip: -12 % bits at -0.14 dB at fixed QP 27, +0.02 dB at equal bitrate
                                       * under the rate controller) */
    int32_t chroma_modes;             /* 1 (default): 2Nx2N intra CUs choose intra_chroma_pred_mode among DM / planar / vertical / horizontal /
                                       * DC by SATD over Cb + Cr; 0: always DM */
    /* ---- one picture over several devices (BASELINE configs[4]): a session may code ONE SLICE — a full-width band of CTU rows — of
     * pictures pic_height high.  `height` is then the band's own height (32 x its CTU rows, the last band takes what is left), the
     * parameter sets describe the whole picture and are identical in every slice's session, the slice header carries the band's
     * slice_segment_address, in-loop filters stop at slice boundaries (pps_loop_filter_across_slices_enabled_flag = 0) and motion
     * vectors never reach across them (nothing is exchanged between the devices).  slice_count = 0 / 1: whole pictures. */
    int32_t pic_height;               /* height of the whole picture (display); used when slice_count > 1 */
    int32_t slice_count, slice_index;
    int32_t slice_ctu_rows[16];       /* CTU rows of every slice, top to bottom (sum = ceil(pic_height / 32)) */
    int32_t rate_share_q16;           /* share of vbv-maxrate / vbv-bufsize this slice plans with, 65536 = all (0 = all) */
    int32_t scenecut;                 /* 1 (default): an IDR picture where the picture changes (mean absolute difference of consecutive source pictures),
                                       * at least min_keyint pictures after the last one (x265 scenecut / min-keyint); 0: IDR every keyint pictures only */
    int32_t gop_balance;              /* 1 (default): a run of pictures between scene cuts / chunk ends is coded as the fewest GOPs keyint allows, of
                                       * near-equal length (300 pictures at keyint 90: IDR at 0, 75, 150, 225), so the GOP lanes of the device pipeline finish
                                       * together; 0: IDR every keyint pictures (0, 90, 180, 270).  The number of IDR pictures is the same either way */
    int32_t rdo_cg;                   /* k > 0: RD zero-out of the 4x4 coefficient groups of inter TUs ("RDOQ-lite"): a group of levels is dropped when the
                                       * squared error it removes is worth less than lambda x k / 2 x its bits.  Default 0 (off): over whole GOPs of the bench
                                       * clip it buys nothing that a higher QP would not (k = 2: -0.6 % bits / -0.006 dB, k = 5: -8.5 % / -0.16 dB at QP 27) */
    /* ---- ABI 3 ---- */
    int32_t p_tiles;                  /* P pictures as a uniform tile grid of their own (PPS 0), one CABAC substream and ONE HOST JOB per tile: what lets the host keep up
                                       * with the device when few pictures are in flight (4320p: one GOP lane, 1.5 Mbit of CABAC per picture; x265 gets the same from WPP
                                       * under `-threads 0`, core/transcoder.py:410-411).  -1 (default): one tile per 1920x1080 of picture (4320p 4x4, 2160p 2x2, up to
                                       * 1080p-class none: tiles that large cost ~0.2 % bits); 0: off; 1: as -1 but at least 2x2 when the level allows.  Motion
                                       * compensation, deblocking and SAO cross tile boundaries; merge / AMVP candidates and CABAC contexts do not */
    int32_t bframes;                  /* 0 (default) / 1 / -1.  1: every second picture of a closed GOP is a B picture between two anchors (x265 bframes; the reference's
                                       * preset=slow runs 4 with b-adapt, core/transcoder.py:399): coding order I0 P2 b1 P4 b3 ..., a B picture predicts from the anchor
                                       * before it (list 0), the one after it (list 1) or both (8.5.3.3.4.2), is never a reference itself (TRAIL_N) and takes QP + 2.
                                       * Packets come out in DECODING order with dts <= pts (mihevc_receive_packet), the MP4 writer adds the ctts box.
                                       * -1: decided per chunk (x265 b-adapt in spirit): a probe on the 1/4-size SOURCE pictures compares how well a picture is
                                       * matched by the picture one place and two places before it; B pictures where two places back is nearly as good (static and
                                       * translating content), none where it is not (zoom, fades: there anchors two pictures apart cost more than B pictures save).
                                       * mihevc_stats.reserved[0..2]: the last probe's two costs (1/1000 per CTU) and its decision */
    int32_t b_qp_offset;              /* QP of a B picture above the anchors around it; -1 (default): 2 (x265 pbratio 1.3) */
    int32_t slice_halo;               /* slice_count > 1 only.  1: the sessions of one picture's slices EXCHANGE rows (they find each other through slice_group and must
                                       * live in one process): the PAD rows of the final reconstruction either side of every seam, so motion vectors cross seams as in a
                                       * whole picture, and 8 rows of the pre-deblock reconstruction + one row of CU records, so deblocking and SAO run across the seams
                                       * (pps_loop_filter_across_slices_enabled_flag = 1); rate control takes its inputs summed over the slices: one plan per picture.
                                       * Point-to-point pulls out of the neighbour's device memory (xGMI peer access), no collective.  0: nothing is exchanged — motion
                                       * constrained slices, filters stop at the seams, every slice its own rate controller (round 2: -1.5 dB at 4320p over 8) */
    int32_t slice_group;              /* slice_halo: any non-zero number shared by the sessions of one picture's slices and by nobody else in the process */
    /* ---- ABI 4 ---- */
    int32_t sign_hide;                /* 1: sign data hiding (sign_data_hiding_enabled_flag in both PPS, x265 signhide): in every 4x4 coefficient group whose first and last
                                       * levels lie more than 3 scan positions apart, the first level's sign is not coded but carried by the parity of the group's
                                       * absolute sum; the kernels adjust one level per group where the parity disagrees (the cheapest +-1 by rounding error).  Every
                                       * path that produces coded levels does it.  The host coder checks the rule in every group it codes and fails the picture with
                                       * MIHEVC_EINVAL when one breaks it.  0 (default): off.  Any other value: MIHEVC_EINVAL at open and in mihevc_write_parameter_sets */
    /* ---- ABI 5 ---- */
    int32_t pic_hash;                 /* decoded picture hash SEI (x265 hash): every access unit carries, in a suffix SEI NAL unit (type 40, payloadType 132) behind its
                                       * slice, a hash of each colour component of the encoder's final reconstruction over the CODED size, which any conforming decoder
                                       * can check the picture it decodes against.  0 (default): off; 1 MD5 (the final picture is copied to pinned host memory and hashed by
                                       * the CABAC job: a verification mode, host-bound); 2 CRC; 3 checksum (both on the device, on the copy stream beside the next step).
                                       * Any other value, or a value != 0 with slice_count > 1: MIHEVC_EINVAL at open and in mihevc_write_parameter_sets */
    /* ---- ABI 6 ---- */
    int32_t ssim;                     /* per-picture SSIM on the device (x265 ssim): 1 = every picture's source is compared with its final reconstruction (after deblocking
                                       * and SAO: what a decoder outputs) over the CODED size, per colour component, by two small launches per step on the copy stream; the
                                       * results come with mihevc_get_frame_quality and mihevc_stats.ssim_*.  The metric: SSIM on 8x8 windows at stride 4 with biased
                                       * variances, C1 = (0.01 peak)^2, C2 = (0.03 peak)^2, in integers up to one double division per window, each window's value rounded
                                       * to a multiple of 2^-32 and summed as int64 (csrc/kernels/ssim.h has it step by step): bit-exact and independent of scheduling.  It
                                       * is the textbook form, not digit for digit the figure libx265 prints.  No bit of the stream and no decision depends on it.
                                       * 0 (default): off, nothing is launched or allocated.  Any other value, or 1 with slice_count > 1 (windows cross the seams): MIHEVC_EINVAL
                                       * at open and in mihevc_write_parameter_sets */
} mihevc_config;

typedef struct mihevc_session mihevc_session;

typedef struct mihevc_stats {
    int64_t frames_in, frames_out, bytes_out;
    double  sse_y, sse_u, sse_v;      /* encoder reconstruction vs source (summed over frames_out), for PSNR */
    double  device_ms, entropy_ms;    /* accumulated device time (HIP events) and host CABAC time (sum over threads) */
    int32_t last_qp;
    int32_t reserved[7];              /* [0..2]: cfg.bframes = -1, the last probe; [3..5]: host microseconds of the chunks in front of their first launch, behind their last
                                       * kernel (last symbol copies + the entropy coding still open), and in all: where wall time that is not device time goes;
                                       * [6]: P/B steps that ran as two lane groups on two streams (0: one launch sequence, e.g. MIHEVC_LANE_GROUPS=1 in the environment at open) */
    /* per-stage device time, filled when cfg.profile_stages: sum of HIP-event intervals and number of launches.
     * index: 0 intra (plan + the anti-diagonal chain of a step), 1 me_search, 2 inter_ctu, 3 deblock (V+H; only without SAO: with SAO the loop filter is one kernel, counted
     * under 4), 4 sao (the whole loop filter: deblock of the CTU's tile + decide + apply + squared error), 5 border pad, 6 unused since ABI 2 (the SSE fold runs on the copy
     * stream), 7 intra second pass of P pictures (two rounds).  One launch covers `pictures` pictures (the lock-step batch). */
    double  stage_ms[8];
    int64_t stage_launches[8];
    int64_t stage_pictures[8];
    /* ---- ABI 6 ---- */
    double  ssim_y, ssim_u, ssim_v;   /* cfg.ssim: sum of the per-picture SSIM over the pictures counted in sse_* (mean = / frames_out once every packet is out), formed from the exact
                                       * integer sum of mihevc_get_frame_quality's ssim_q32 over those pictures: / (ssim_windows * 2^32); 0 when off */
} mihevc_stats;

int  mihevc_abi_version(void);
int  mihevc_device_count(void);                      /* gfx950 devices visible; 0 when none / no runtime */
/* NUMA node of the host memory closest to `device` (its PCI function's numa_node in sysfs); -1 when the platform does not say.  A process that
 * drives one device (one process per GPU: bench.py, hevc_amd/batch.py) binds itself to that node's CPUs BEFORE its first mihevc_open, so the pinned
 * symbol buffers and the CABAC workers that read them sit next to the device (hevc_amd/utils.py: bind_to_device_node). */
int  mihevc_device_numa_node(int device);
void mihevc_config_default(mihevc_config *cfg);      /* 1080p30 8-bit SDR at the reference's operating point */
int  mihevc_open(const mihevc_config *cfg, int device, mihevc_session **out);
/* Caller-owned host planes (8-bit: 1 byte/sample, 10-bit: 2 bytes little endian), copied/uploaded before return. */
int  mihevc_send_frame(mihevc_session *s, const void *y, const void *u, const void *v,
                       int pitch_y, int pitch_c, int64_t pts);
/* The same without waiting for the upload: the copies are enqueued on the session's side stream and the call returns.  The caller's planes must stay
 * valid and unmodified until mihevc_sync_uploads() or mihevc_flush() has returned (a decoder that feeds the session from a ring of N frame buffers calls
 * mihevc_sync_uploads before it reuses the oldest).  For the copies to run as DMA beside the caller the planes have to be page-locked host memory
 * (hipHostMalloc / hipHostRegister; torch: pin_memory()); with pageable memory the call is correct but as slow as mihevc_send_frame. */
int  mihevc_send_frame_async(mihevc_session *s, const void *y, const void *u, const void *v,
                             int pitch_y, int pitch_c, int64_t pts);
int  mihevc_sync_uploads(mihevc_session *s);         /* every frame handed over so far has left the caller's buffers */
/* Frames already resident in device memory (same layout, device pointers): the benchmark path.  Stream ordering contract: the copy
 * into the session's own pitch-aligned picture is ENQUEUED on the session's stream and the call returns before it has run, and it is not
 * ordered against any stream of the caller.  So (1) the producer of y/u/v must have finished before the call (synchronise its stream or
 * event first), and (2) the three planes must stay valid and unmodified until the picture's packet has been received, or mihevc_flush
 * has returned, whichever comes first (host buffers of mihevc_send_frame may be reused as soon as that call returns).  When the display size
 * already is the coded size (multiples of 8) and planes / pitches are 4-byte aligned the session codes straight from the caller's planes. */
int  mihevc_send_frame_device(mihevc_session *s, const void *y, const void *u, const void *v,
                              int pitch_y, int pitch_c, int64_t pts);
/* n pictures that are ALREADY in device memory in one call (pts = first_pts, first_pts + 1, ...): mihevc_send_frame_device n times, for a caller that holds the pointers
 * in arrays anyway — a host language's call overhead (ctypes: ~3.5 us per call, 1 ms per 300-frame clip at 5000 fps) stays out of the loop.  Same ownership rules; stops
 * at the first error.  Chunks that fill up on the way are coded inside the call, as with the one-picture form. */
int  mihevc_send_frames_device(mihevc_session *s, int n, const void *const *y, const void *const *u, const void *const *v,
                               int pitch_y, int pitch_c, int64_t first_pts);
/* ---- added under ABI 6: sources that are not the session's own layout (symbols only: no existing struct or function changes) ----
 * A picture of the session's DISPLAY size in another sample layout, converted on the device into the session's planar 4:2:0 planes at cfg.bit_depth
 * (hevc_amd/csrc/kernels/ingest.h states the arithmetic; DESIGN.md repeats it): 4:2:2 and 4:4:4 chroma is filtered down (the siting of
 * chroma_sample_loc_type 0), deeper samples are rounded half up once, shallower ones shifted up, values above 2^bit_depth - 1 in an lsb-aligned plane are
 * clamped.  Covers ffmpeg's yuv420p / yuv422p / yuv444p (and yuvj*), yuv4xxp{9,10,12,14,16}le, nv12 / nv16 / nv24, p010le / p016le / p210le / p216le /
 * p410le / p416le.  Not covered (MIHEVC_EINVAL; hevc_amd._lib.src_format_for gives None): swapped semi-planar (nv21), packed formats (yuyv422, uyvy422,
 * v210), 4:1:1 / 4:1:0, big endian, alpha; there is no range conversion.  RGB / gbrp sources: mihevc_send_frame_rgb below. */
typedef struct mihevc_src_format {
    int32_t chroma;        /* 420, 422, 444 */
    int32_t semi_planar;   /* 0: y, u, v planes; 1: y + interleaved CbCr in u (Cb in the even elements), v is ignored */
    int32_t bit_depth;     /* significant bits 8..16; > 8: little-endian uint16 elements */
    int32_t msb_aligned;   /* 1 (bit_depth > 8 only): the bits sit at the top of the word (P010 ...) */
    int32_t reserved[4];   /* 0 */
} mihevc_src_format;

#define MIHEVC_SRC_DEVICE 1   /* y/u/v are device pointers */
#define MIHEVC_SRC_ASYNC  2   /* return with the upload in flight (the rules of mihevc_send_frame_async) */

/* pitch_y, pitch_c: in elements of the plane (an interleaved plane: >= twice the chroma width).  Host planes are copied as they are into a staging set of
 * the session and converted from there; without MIHEVC_SRC_ASYNC the caller's planes may be reused on return.  With MIHEVC_SRC_DEVICE the kernel reads the
 * caller's planes where they are: their producer must have finished before the call, and they must stay valid and unmodified until mihevc_sync_uploads or
 * mihevc_flush has returned (for every format: the planes are always copied or converted, never coded where they lie).  A format that already is the session's layout (420, planar, bit_depth == cfg.bit_depth, not msb_aligned) gives the byte-identical
 * stream of mihevc_send_frame.  MIHEVC_EINVAL, decided before any device call and leaving the session usable: NULL fmt, chroma other than the three values,
 * bit_depth outside 8..16, msb_aligned with 8 bits, non-zero reserved, odd cfg.width / cfg.height, a pitch smaller than the plane, unknown flag bits,
 * slice_count > 1.  MIHEVC_ESTATE after flush. */
int  mihevc_send_frame_fmt(mihevc_session *s, const mihevc_src_format *fmt, const void *y, const void *u, const void *v,
                           int pitch_y, int pitch_c, int64_t pts, int flags);
/* ---- added under ABI 6: RGB sources (symbols only) ----
 * A full-range R'G'B' picture of the session's DISPLAY size, planar or packed, integers of 8 .. 16 significant bits (lsb aligned; uint8 at 8 bit, else
 * little-endian uint16; values above 2^bit_depth - 1 are clamped) or IEEE half / single floats in [0, 1] (planes only; clamped, NaN is 0).  One kernel
 * launch applies the colour matrix, scales to the limited or full range of cfg.bit_depth, filters chroma down to 4:2:0 (the siting and taps of the 4:4:4 case
 * of mihevc_send_frame_fmt) and fills the margin; hevc_amd/csrc/kernels/ingest_rgb.h states the integer arithmetic, DESIGN.md 6d repeats it.  Covers ffmpeg's
 * gbrp, gbrp{9,10,12,14,16}le, gbrpf32le, rgb24 / bgr24, rgba / bgra / argb / abgr / rgb0 / bgr0 / 0rgb / 0bgr, rgb48le / bgr48le, rgba64le / bgra64le
 * (hevc_amd._lib.rgb_format_for).  A fourth element of a packed pixel is ignored.  Neither the session's signalled matrix nor its range changes: the caller opens
 * the session with the cfg.matrix / cfg.full_range it wants in the stream, and matrix = 0 / range = 0 here follow them. */
typedef struct mihevc_rgb_format {
    int32_t layout;      /* 0 three planes; 3 / 4: packed, that many elements per pixel */
    int32_t r, g, b;     /* planar: which of p0..p2 holds the component; packed: its element index inside the pixel */
    int32_t sample;      /* 0 unsigned integer, 1 IEEE half, 2 IEEE single (layout 0 only) */
    int32_t bit_depth;   /* sample 0: 8..16; floats: 0 */
    int32_t matrix;      /* 0: the session's cfg.matrix; else 1, 5, 6, 9 */
    int32_t range;       /* 0: the session's cfg.full_range; 1 limited; 2 full */
    int32_t reserved[4]; /* 0 */
} mihevc_rgb_format;
/* pitch: elements per row, the same for every plane (a packed plane: >= layout * width).  Ownership, staging, stream ordering and flags are those of
 * mihevc_send_frame_fmt: host planes are copied into the session's staging set and converted from there, and without MIHEVC_SRC_ASYNC they may be reused on
 * return; with MIHEVC_SRC_DEVICE the kernel reads the planes where they are, and they must stay valid and unmodified until mihevc_sync_uploads or mihevc_flush
 * has returned.  A packed source has one plane, p0; p1 and p2 are not read.  MIHEVC_EINVAL, decided before any device call and leaving the session usable: a
 * NULL fmt or a NULL plane the layout needs, a plane whose address is not a multiple of the element size, a layout other than 0 / 3 / 4, component
 * indices out of range or not distinct, a depth outside 8..16 (floats: other than 0), floats with a packed layout, non-zero reserved, a matrix that resolves to
 * anything other than 1 / 5 / 6 / 9 (a session whose cfg.matrix is 0 or 2 with matrix = 0 included), a range above 2, odd cfg.width / cfg.height, a pitch smaller
 * than the row, unknown flag bits, slice_count > 1.  MIHEVC_ESTATE after flush. */
int  mihevc_send_frame_rgb(mihevc_session *s, const mihevc_rgb_format *fmt, const void *p0, const void *p1, const void *p2,
                           int pitch, int64_t pts, int flags);
/* ---- added under ABI 6: sources through a COLOUR TABLE (symbols only) ----
 * A 3D lookup table with tetrahedral interpolation between the source's colours and the session's: an HDR master into an SDR stream, log footage into Rec.709, a
 * grade shipped as a .cube file.  The source is a planar 4:2:0 Y'CbCr picture of the session's DISPLAY size at 8, 10 or 12 bit (uint8 at 8 bit, else little-endian
 * uint16, lsb aligned, values above 2^bit_depth - 1 clamped) with its own matrix and range.  One kernel launch brings chroma to the luma grid, converts to
 * R'G'B' at 16 bit, looks every pixel up in the table and goes on as mihevc_send_frame_rgb does for a 16-bit source: the session's matrix and range, cfg.bit_depth,
 * 4:2:0, margin.  Integers throughout; hevc_amd/csrc/kernels/lut3d.h states the arithmetic, DESIGN.md 6i repeats it.  Not covered: RGB, 4:2:2 and 4:4:4 sources,
 * 1D shaper tables, other interpolations, per-scene tone mapping, scaling, deinterlacing or denoising in the same pass, sliced sessions.
 *
 * mihevc_set_lut3d: table holds n^3 x 3 uint16 in host memory in the order of a .cube file, table[((b * n + g) * n + r) * 3 + c], input and output 0 .. 65535 for
 * 0.0 .. 1.0; it is copied before the call returns.  The table may be replaced between frames: frames already sent keep the table they were sent under (the copy
 * is ordered behind their launches on the upload stream; the device is not waited for).  table == NULL drops the table.  MIHEVC_EINVAL: n outside 2 .. 65 with a
 * table, slice_count > 1. */
int  mihevc_set_lut3d(mihevc_session *s, int n, const uint16_t *table);
typedef struct mihevc_lut3d_src {
    int32_t bit_depth;    /* 8, 10 or 12 */
    int32_t matrix;       /* of the source: 1, 5, 6 or 9 */
    int32_t full_range;   /* of the source: 0 limited, 1 full */
    int32_t reserved[4];  /* 0 */
} mihevc_lut3d_src;
/* pitch_y, pitch_c: in elements.  Flags, staging, ownership and stream ordering are those of mihevc_send_frame_fmt.  The output matrix and range are the
 * session's cfg.matrix and cfg.full_range, as mihevc_send_frame_rgb resolves them with matrix = 0 and range = 0.  MIHEVC_EINVAL, decided before any device call
 * and leaving the session usable: NULL src or plane, a depth other than 8 / 10 / 12, a source matrix other than 1 / 5 / 6 / 9, full_range outside {0, 1}, non-zero
 * reserved, no table set, a cfg.matrix other than 1 / 5 / 6 / 9, odd cfg.width / cfg.height, a pitch smaller than the plane, a plane whose address is not a
 * multiple of the element size, unknown flag bits, slice_count > 1.  MIHEVC_ESTATE after flush.  The entry keeps no ring: it mixes with mihevc_send_frame and
 * mihevc_send_frame_fmt as they mix with each other. */
int  mihevc_send_frame_lut3d(mihevc_session *s, const mihevc_lut3d_src *src, const void *y, const void *u, const void *v,
                             int pitch_y, int pitch_c, int64_t pts, int flags);
/* ---- added under ABI 6: sources of another SIZE (symbols only) ----
 * A planar 4:2:0 picture of src->width x src->height samples at src->bit_depth, scaled down on the device into the session's planes of cfg.width x cfg.height
 * at cfg.bit_depth by a separable 16-tap polyphase Catmull-Rom filter with an exact integer definition (hevc_amd/csrc/kernels/scale.h and
 * hevc_amd/csrc/scale_taps.h state the arithmetic).  Per axis cfg size <= source size <= 4 x cfg size, the axes independent; equal sizes give the conversion of
 * mihevc_send_frame_fmt for a planar 4:2:0 source.  Elements are uint8 at 8 bit, else little-endian uint16, lsb aligned, values above 2^bit_depth - 1 clamped;
 * chroma is sited as chroma_sample_loc_type 0 on both sides.  No sample aspect ratio is signalled: the caller chooses sizes of one shape. */
typedef struct mihevc_scale_src {
    int32_t width, height;   /* the source picture: both even, >= 16 */
    int32_t bit_depth;       /* significant bits 8..16 */
    int32_t reserved[5];     /* 0 */
} mihevc_scale_src;
/* pitch_y, pitch_c: in elements.  Flags, ownership, staging and stream ordering are those of mihevc_send_frame_fmt: host planes are copied into the session's
 * staging set and scaled from there, and without MIHEVC_SRC_ASYNC they may be reused on return; with MIHEVC_SRC_DEVICE the kernel reads the planes where they
 * are (several sessions may read the same planes), and they must stay valid and unmodified until mihevc_sync_uploads or mihevc_flush has returned.
 * MIHEVC_EINVAL, decided before any device call and leaving the session usable: NULL src or plane, odd sizes or sizes below 16 (cfg.width / cfg.height
 * included), a size ratio outside [1, 4] on either axis, bit_depth outside 8..16, non-zero reserved, a pitch smaller than the plane, unknown flag bits,
 * slice_count > 1.  MIHEVC_ESTATE after flush. */
int  mihevc_send_frame_scaled(mihevc_session *s, const mihevc_scale_src *src, const void *y, const void *u, const void *v,
                              int pitch_y, int pitch_c, int64_t pts, int flags);
/* ---- added under ABI 6: INTERLACED sources (symbols only) ----
 * A woven interlaced frame of the session's DISPLAY size, planar 4:2:0 at cfg.bit_depth (uint8 at 8 bit, else little-endian uint16, values above
 * 2^bit_depth - 1 clamped), deinterlaced on the device into progressive pictures by a motion-adaptive, edge-directed filter in the manner of yadif with an exact
 * integer definition (hevc_amd/csrc/kernels/deint.h states the arithmetic).  The rows of one field are kept, the others are interpolated from the
 * frame before, the frame itself and the frame after; the first frame stands in for its missing predecessor and the last one for its missing successor.
 * Frame-rate mode gives one picture per frame (the first field's rows kept), field-rate mode two: the first field's with the frame's pts, the second field's with
 * pts + 1, so the caller numbers pts in field periods and opens the session at twice the frame rate.  The stream stays progressive (HEVC has no interlaced
 * coding tools).  Inverse telecine and field matching: mihevc_send_frame_fieldmatch.  Not covered: other filters, other layouts or depths than the session's, scaling in the same pass,
 * parity changes inside a clip, sliced sessions, pic_struct signalling. */
typedef struct mihevc_deint {
    int32_t tff;          /* 1: top field first, 0: bottom field first */
    int32_t field_rate;   /* 0: one picture per frame; 1: two (pts, pts + 1) */
    int32_t reserved[6];  /* 0 */
} mihevc_deint;
/* pitch_y, pitch_c: in elements.  The frame is copied into a ring of three source-size pictures the session owns (allocated at the first call), host planes on
 * the upload stream, device planes device to device.  Flags and ownership are those of mihevc_send_frame_fmt: host planes may be reused on return unless
 * MIHEVC_SRC_ASYNC is set, device planes (MIHEVC_SRC_DEVICE) after mihevc_sync_uploads or mihevc_flush.  A frame's picture(s) are produced when the NEXT frame
 * arrives, the last frame's by mihevc_flush; mihevc_stats.frames_in counts pictures.  MIHEVC_EINVAL, decided before any device call and leaving the session
 * usable: NULL d or plane, tff or field_rate outside {0, 1}, non-zero reserved, a tff or field_rate other than that of the session's first deinterlaced frame,
 * cfg.width odd, cfg.height not a multiple of 4, either below 16, a pitch smaller than the plane, unknown flag bits, slice_count > 1.  MIHEVC_ESTATE after
 * flush; and every OTHER entry that sends a frame returns MIHEVC_ESTATE while a deinterlaced frame is pending (sent, its pictures not yet produced). */
int  mihevc_send_frame_deint(mihevc_session *s, const mihevc_deint *d, const void *y, const void *u, const void *v,
                             int pitch_y, int pitch_c, int64_t pts, int flags);
/* ---- added under ABI 6: NOISY sources (symbols only) ----
 * A progressive frame of the session's DISPLAY size, planar 4:2:0 at cfg.bit_depth (uint8 at 8 bit, else little-endian uint16, values above 2^bit_depth - 1
 * clamped), denoised on the device by a motion-adaptive spatio-temporal filter with an exact integer definition (hevc_amd/csrc/kernels/denoise.h
 * states the arithmetic): every output sample is a weighted mean of the sample, its eight neighbours and the co-sited samples of the frame before and the frame
 * after, each weight a threshold minus a difference, so that edges, impulses and moving areas pass as they are.  The first frame stands in for its missing
 * predecessor and the last one for its missing successor.  The four strengths are thresholds in 8-bit units (shifted left by bit_depth - 8); all zero leaves the
 * frame as it is.  Not covered: motion-compensated or block-matching filters, other layouts or depths than the session's, scaling, deinterlacing or RGB in the
 * same session, sliced sessions, noise-level estimation. */
typedef struct mihevc_denoise {
    int32_t luma_spatial, luma_temporal;       /* 0 .. 255 */
    int32_t chroma_spatial, chroma_temporal;   /* 0 .. 255 */
    int32_t reserved[4];                       /* 0 */
} mihevc_denoise;
/* pitch_y, pitch_c: in elements.  The frame is copied into the ring of three source-size pictures that mihevc_send_frame_deint uses too; flags and ownership are
 * those of mihevc_send_frame_deint.  A frame's picture is produced when the NEXT frame arrives, the last frame's by mihevc_flush; mihevc_stats.frames_in counts
 * pictures.  The strengths sent with a frame apply to that frame's picture and may change from frame to frame.  MIHEVC_EINVAL, decided before any device call
 * and leaving the session usable: NULL d or plane, a strength outside 0 .. 255, non-zero reserved, cfg.width or cfg.height odd or below 16, a pitch smaller than
 * the plane, unknown flag bits, slice_count > 1.  MIHEVC_ESTATE after flush; every OTHER entry that sends a frame, mihevc_send_frame_deint included, returns
 * MIHEVC_ESTATE while a denoised frame is pending (sent, its picture not yet produced), and this one does while a deinterlaced frame is pending. */
int  mihevc_send_frame_denoise(mihevc_session *s, const mihevc_denoise *d, const void *y, const void *u, const void *v,
                               int pitch_y, int pitch_c, int64_t pts, int flags);
/* ---- added under ABI 6: TELECINED sources (symbols only) ----
 * Woven frames of the session's DISPLAY size, planar 4:2:0 at cfg.bit_depth (uint8 at 8 bit, else little-endian uint16, values above 2^bit_depth - 1 clamped),
 * that carry film in fields (3:2 pulldown): inverse telecine on the device with an exact integer definition (hevc_amd/csrc/kernels/fieldmatch.h
 * states the metrics, hevc_amd/csrc/fieldmatch_plan.h the decisions).  Field matching: the rows of the declared first field of a frame are kept and woven with
 * the other rows of the frame itself (c), of the frame before (p) or of the frame after (n), whichever combs least; nothing is interpolated.  deint: a frame
 * whose best match is still combed (video passages, orphan fields at edits) becomes the picture mihevc_send_frame_deint gives in frame-rate mode.  decimate:
 * of every cycle of five frames, counted from the first, the one that differs least from the frame before it is dropped; the j-th picture that comes out takes
 * pts_first + j, so the caller opens the session at 4/5 of the source rate; a last cycle of fewer than five frames comes out whole.  Without decimate a picture
 * takes its frame's pts.  Not covered: other cadences and variable cycles, variable-frame-rate output, blended fields, pic_struct signalling, scaling, denoising
 * or RGB in the same session, sliced sessions. */
typedef struct mihevc_fieldmatch {
    int32_t tff;          /* 1: top field first, 0: bottom field first (the DECLARED order; the n match serves a clip whose order is the opposite) */
    int32_t decimate;     /* 1: drop one frame of every five */
    int32_t deint;        /* 1: deinterlace frames that stay combed */
    int32_t reserved[5];  /* 0 */
} mihevc_fieldmatch;
/* pitch_y, pitch_c: in elements.  The frame is copied into the ring of three source-size pictures that mihevc_send_frame_deint uses too; flags and ownership are
 * those of mihevc_send_frame_deint.  Frame k is decided when frame k + 1 arrives, the last frame by mihevc_flush: its metrics are taken on the device, the call
 * waits for them (and so for everything sent before, the new frame's upload included: with MIHEVC_SRC_ASYNC it returns with less in flight than the other
 * entries do) and launches the picture.  With decimate the pictures of the open cycle are held until its fifth frame is decided.  mihevc_stats.frames_in counts
 * pictures.  MIHEVC_EINVAL, decided before any device call and leaving the session usable: NULL d or plane, a field of d outside {0, 1}, non-zero reserved, a
 * mode other than that of the session's first fieldmatch frame, cfg.width odd, cfg.height not a multiple of 4, either below 16, a pitch smaller than the plane,
 * unknown flag bits, slice_count > 1.  MIHEVC_ESTATE after flush, and while a deinterlaced or denoised frame is pending; every OTHER entry that sends a frame
 * returns MIHEVC_ESTATE from the first fieldmatch frame until flush. */
int  mihevc_send_frame_fieldmatch(mihevc_session *s, const mihevc_fieldmatch *d, const void *y, const void *u, const void *v,
                                  int pitch_y, int pitch_c, int64_t pts, int flags);
typedef struct mihevc_fm_frame {
    uint64_t comb_sum[3];     /* S_c, S_p, S_n */
    uint32_t comb_block[3];   /* K_c, K_p, K_n */
    uint64_t dup_sum;         /* DS (the first frame: all-ones) */
    uint32_t dup_block;       /* DB (the first frame: all-ones) */
    int32_t match;            /* 0 c, 1 p, 2 n */
    int32_t deinterlaced;     /* 1: the picture is the deinterlacer's */
    int32_t dropped;          /* 1: decimated */
    int64_t picture;          /* output index, -1 dropped */
} mihevc_fm_frame;
/* What was decided for fieldmatch frame `frame` (0-based, in the order sent).  MIHEVC_EAGAIN until it is decided: the frame has arrived but the next one (or
 * flush) has not, or, with decimate, its cycle is still open; MIHEVC_EINVAL: NULL, or a frame that was never sent. */
int  mihevc_get_fieldmatch_info(mihevc_session *s, int64_t frame, mihevc_fm_frame *out);
/* ---- added under ABI 6: FRAME-RATE MULTIPLICATION (symbols only) ----
 * Progressive frames of the session's DISPLAY size, planar 4:2:0 at cfg.bit_depth (uint8 at 8 bit, else little-endian uint16, values above 2^bit_depth - 1
 * clamped), between which factor - 1 pictures are interpolated on the device with an exact integer definition (hevc_amd/csrc/kernels/mcfi.h
 * states the arithmetic).  Mode mc: one bilateral vector per 8x8 luma block from a two-level block search (+-36 luma samples of motion per frame), smoothed by a
 * 3x3 median, zeroed where it does not beat the zero vector; the pictures are rendered with overlapped blocks and bilinear fetches from both frames; a pair whose
 * mean absolute luma difference exceeds scene_threshold (8-bit units; 0: no check) is a scene cut and repeats its nearer frame instead.  Mode blend: the weighted
 * mean of the two frames.  Not covered: sub-sample vectors, wider ranges, occlusion reasoning, variable block sizes, arbitrary output rates and rate reduction,
 * scaling, deinterlacing, denoising, inverse telecine, RGB or colour tables in the same session, sliced sessions, other layouts or depths than the session's. */
typedef struct mihevc_interpolate {
    int32_t factor;            /* 2, 3 or 4: pictures per frame */
    int32_t mode;              /* 0: motion compensated, 1: blend */
    int32_t scene_threshold;   /* 0 .. 255, 0: off (10 is a fair default) */
    int32_t reserved[5];       /* 0 */
} mihevc_interpolate;
/* pitch_y, pitch_c: in elements.  The frame is copied into the ring of three source-size pictures that mihevc_send_frame_deint uses too; flags and ownership are
 * those of mihevc_send_frame_deint.  When frame k + 1 arrives, frame k yields its `factor` pictures at pts_k + j, j = 0 .. factor - 1: the caller numbers pts in
 * the session's time base with consecutive frames `factor` apart and opens the session at factor times the source rate.  mihevc_flush gives the last frame's
 * j = 0 picture only: n frames give factor (n - 1) + 1 pictures.  The call never waits for the device on account of the scene check: the render kernel reads the
 * sum itself.  mihevc_stats.frames_in counts pictures.  MIHEVC_EINVAL, decided before any device call and leaving the session usable: NULL d or plane, a factor
 * outside 2 .. 4, a mode outside {0, 1}, a scene_threshold outside 0 .. 255, non-zero reserved, a factor or mode other than that of the session's first
 * interpolated frame, cfg.width or cfg.height odd or below 16, a pitch smaller than the plane, unknown flag bits, slice_count > 1.  MIHEVC_ESTATE after flush,
 * and while a frame of another ring entry is pending; every OTHER entry that sends a frame returns MIHEVC_ESTATE while an interpolated frame is pending. */
int  mihevc_send_frame_interpolate(mihevc_session *s, const mihevc_interpolate *d, const void *y, const void *u, const void *v,
                                   int pitch_y, int pitch_c, int64_t pts, int flags);
/* ---- added under ABI 6: sources SMALLER than the session (symbols only) ----
 * A planar 4:2:0 picture of src->width x src->height samples at src->bit_depth, enlarged on the device into the session's planes of cfg.width x cfg.height at
 * cfg.bit_depth, with an exact integer definition (hevc_amd/csrc/kernels/upscale.h and hevc_amd/csrc/scale_taps.h state the arithmetic): separable
 * 4-tap Catmull-Rom interpolation at the positions of mihevc_send_frame_scaled (the cubic is not stretched), after each pass a blend of `antiring` eighths towards
 * the range of the two samples around the position (8: the result never leaves it, so an edge grows no halo; 0: the plain cubic), then on luma a 3x3 sharpener of
 * gain `sharpen` sixteenths (centre against a 1-2-1 blur) whose result is clamped to the range of its 3x3 neighbourhood, so it cannot overshoot (0: off).  Per
 * axis source size <= cfg size <= 4 x source size, the axes independent; equal sizes with sharpen 0 give the conversion of mihevc_send_frame_fmt for a planar
 * 4:2:0 source.  Elements are uint8 at 8 bit, else little-endian uint16, lsb aligned, values above 2^bit_depth - 1 clamped; chroma is sited as
 * chroma_sample_loc_type 0 on both sides.  The constants (cubic, clamp to the two nearest samples, the blur, the gain scale) are a proposal and were not tuned.
 * Not covered: learned super-resolution, edge-directed interpolation, ratios above 4, one axis enlarged and the other reduced, sources that are not planar
 * 4:2:0, the other source filters in the same picture, sliced sessions, sample aspect ratio. */
typedef struct mihevc_upscale_src {
    int32_t width, height;   /* the source picture: both even, >= 16 */
    int32_t bit_depth;       /* significant bits 8..16 */
    int32_t sharpen;         /* 0..64, sixteenths (8 is a fair default) */
    int32_t antiring;        /* 0..8, eighths (8 is a fair default) */
    int32_t reserved[3];     /* 0 */
} mihevc_upscale_src;
/* pitch_y, pitch_c: in elements.  Flags, ownership, staging and stream ordering are those of mihevc_send_frame_scaled.  sharpen and antiring may change from
 * frame to frame; the session keeps the tables of the last source size.  MIHEVC_EINVAL, decided before any device call and leaving the session usable: NULL src
 * or plane, odd sizes or sizes below 16 (cfg.width / cfg.height included), a source larger than the session or smaller than a quarter of it on either axis,
 * bit_depth outside 8..16, sharpen outside 0..64, antiring outside 0..8, non-zero reserved, a pitch smaller than the plane, unknown flag bits, slice_count > 1.
 * MIHEVC_ESTATE after flush. */
int  mihevc_send_frame_upscaled(mihevc_session *s, const mihevc_upscale_src *src, const void *y, const void *u, const void *v,
                                int pitch_y, int pitch_c, int64_t pts, int flags);
/* ---- added under ABI 6: LEARNED super-resolution (symbols only) ----
 * An RRDBNet (the architecture of RealESRGAN_x4plus, RealESRGAN_x2plus and RealESRGANv2-anime_6B: num_feat 64, num_grow_ch 32, `blocks` residual-in-residual
 * dense blocks, scale 4 or 2) evaluated on the device with half activations and weights and fp32 sums on the matrix unit; DESIGN.md 6l is the numerical
 * definition, hevc_amd/csrc/sr_net.h the flat order of the weights (hevc_amd.sr.load_rrdbnet produces it from a .pth file).  No weights ship with the library.
 * The compact networks (SRVGGNetCompact: realesr-animevideov3, realesr-general-x4v3 with its denoise blend) are mihevc_set_sr_compact below.
 * Not covered: other architectures, scale 3 and 1, other channel counts, tiling and frames too large for
 * device memory, a session larger than the network's output (an enlargement behind the network), 4:2:2 / 4:4:4 / semi-planar / 16-bit Y'CbCr into the
 * network, HDR transfer handling, the other source filters in the same picture, sliced sessions, batching, fp8 / int8 weights, face enhancement. */
typedef struct mihevc_sr_model {
    int32_t scale;           /* 4 or 2 */
    int32_t blocks;          /* RRDBs in the trunk, >= 1 (23 in x4plus / x2plus, 6 in anime_6B) */
    int32_t reserved[6];     /* 0 */
} mihevc_sr_model;
/* The model of the session: weights (count floats, the flat order of sr_net.h) are rounded to half, packed and on their way to the device before the call
 * returns, so the caller's array is free.  model == NULL drops the model.  A model may be replaced between frames under the rule of mihevc_set_lut3d: frames
 * already sent keep the model they were sent under.  MIHEVC_EINVAL: a scale other than 4 / 2, blocks outside 1 .. 64, non-zero reserved, NULL weights, a count
 * other than the model's, slice_count > 1.  MIHEVC_ENOMEM: the device cannot hold the weights; the session has no model then */
int  mihevc_set_sr_model(mihevc_session *s, const mihevc_sr_model *model, const float *weights, size_t count);
/* A full-range R'G'B' picture of src_width x src_height in the layouts of mihevc_send_frame_rgb, enlarged by the model into the session's planes: cfg.width and
 * cfg.height must equal scale x the source size.  The network's output is clamped to [0, 1] and converted as mihevc_send_frame_rgb converts half planes
 * (fmt->matrix and fmt->range as there).  Flags, staging, ownership and stream ordering are those of mihevc_send_frame_rgb; pitch: elements per row of the SOURCE.
 * Device memory for the activations (about 6048 bytes per source pixel at scale 4, a quarter of that at scale 2; sr_net.h states the formula) is allocated at the
 * first frame of a size; nothing is tiled: MIHEVC_ENOMEM when the device cannot hold it, and the session goes on.  MIHEVC_EINVAL, decided before any device
 * call and leaving the session usable: everything mihevc_send_frame_rgb refuses, no model set, a size mismatch, odd source dimensions with scale 2, a source
 * side below 4, slice_count > 1.  MIHEVC_ESTATE after flush.  The entry keeps no ring: it mixes with the other entries that keep none. */
int  mihevc_send_frame_sr(mihevc_session *s, const mihevc_rgb_format *fmt, int src_width, int src_height, const void *p0, const void *p1, const void *p2,
                          int pitch, int64_t pts, int flags);
/* ---- added under ABI 6: learned super-resolution for Y'CbCr sources and to a TARGET SIZE (symbols only) ----
 * The geometry rule of the two entries below, with (nw, nh) = scale x the source size: cfg.width x cfg.height == nw x nh is the direct route of
 * mihevc_send_frame_sr; a session for which per axis nw / 4 <= cfg size <= nw, all four sizes even and at least 16 (the rule of mihevc_send_frame_scaled
 * with the network's output as its source) takes the resized route: the network's output is converted (the session's matrix and range) into an intermediate
 * planar 4:2:0 picture of nw x nh at 10 bit, always, which the scaler of mihevc_send_frame_scaled brings to cfg.width x cfg.height at cfg.bit_depth with its one
 * rounding.  That picture (3 nw nh bytes) lives and dies with the activations, under the same MIHEVC_ENOMEM rule.  Anything else, a session LARGER than the
 * network's output included, is MIHEVC_EINVAL. */
typedef struct mihevc_sr_yuv {
    int32_t width, height;   /* the source picture: both even, >= 4 */
    int32_t bit_depth;       /* 8, 10 or 12 */
    int32_t matrix;          /* of the source: 1, 5, 6 or 9 */
    int32_t full_range;      /* of the source: 0 limited, 1 full */
    int32_t reserved[3];     /* 0 */
} mihevc_sr_yuv;
/* A planar 4:2:0 Y'CbCr picture of src->width x src->height (uint8 at 8 bit, else little-endian uint16, lsb aligned, values above 2^bit_depth - 1 clamped)
 * through the session's model into the session's planes; the session's size under the geometry rule above.  One launch (k_sr_from_yuv;
 * hevc_amd/csrc/kernels/sr_yuv.h states the arithmetic, DESIGN.md 6l repeats it) brings chroma to the luma grid and converts to R'G'B' at 16 bit exactly as
 * mihevc_send_frame_lut3d does in front of its table, and writes the network's input.  The output side uses cfg.matrix and cfg.full_range.  pitch_y, pitch_c: in
 * elements.  Flags, staging, ownership, stream ordering, memory and "keeps no ring" are those of mihevc_send_frame_sr.  MIHEVC_EINVAL, decided before any
 * device call and leaving the session usable, the entry's own arguments first: NULL src or plane, no model set, a depth other than 8 / 10 / 12, a source matrix or
 * a cfg.matrix other than 1 / 5 / 6 / 9, full_range outside {0, 1}, non-zero reserved, odd source sides or sides below 4, a plane whose address is not a multiple
 * of the element size, a pitch smaller than the row, the geometry rule; then unknown flag bits; then odd cfg.width / cfg.height and slice_count > 1; then the
 * code of a failed session; MIHEVC_ESTATE after flush or while a ring entry waits for its next frame. */
int  mihevc_send_frame_sr_yuv(mihevc_session *s, const mihevc_sr_yuv *src, const void *y, const void *u, const void *v, int pitch_y, int pitch_c,
                              int64_t pts, int flags);
/* mihevc_send_frame_sr with the geometry rule above in place of "exactly scale x the source"; everything else, the order of the refusals included, as there
 * and as for mihevc_send_frame_sr_yuv. */
int  mihevc_send_frame_sr_fit(mihevc_session *s, const mihevc_rgb_format *fmt, int src_width, int src_height, const void *p0, const void *p1, const void *p2,
                              int pitch, int64_t pts, int flags);
/* ---- added under ABI 6: COMPACT super-resolution networks (symbols only) ----
 * An SRVGGNetCompact (the architecture of realesr-animevideov3, 16 trunk convolutions, and of realesr-general-x4v3 / realesr-general-wdn-x4v3, 32: num_feat 64,
 * a PReLU with one slope per channel behind every convolution but the last, a pixel-shuffle and the sum with the source enlarged by nearest; scale 4 or 2)
 * evaluated on the device with half activations and weights and fp32 sums on the matrix unit.  DESIGN.md 6m is the numerical definition,
 * hevc_amd/csrc/sr_compact_net.h the flat order of the weights (hevc_amd.sr.load_compact produces it from a .pth file; hevc_amd.sr.blend is the family's denoise
 * strength, a blend of two models' weights on the host).  No weights ship with the library.  Not covered: scale 3 and 1, num_feat other than 64. */
typedef struct mihevc_sr_compact {
    int32_t scale;           /* 4 or 2 */
    int32_t convs;           /* trunk convolutions, 1 .. 64 (16 in animevideov3, 32 in general-x4v3) */
    int32_t reserved[6];     /* 0 */
} mihevc_sr_compact;
/* The model of the session, under the rules of mihevc_set_sr_model: packed and on its way to the device before the call returns, frames already sent keep the
 * model they were sent under.  A session has ONE model of either kind: setting one replaces the other, and mihevc_set_sr_model(s, NULL, ...) drops whichever is
 * set.  mihevc_send_frame_sr, _sr_fit and _sr_yuv run whichever model is set under their own geometry rules, with one difference: a compact network has no
 * pixel-unshuffle, so with a compact model of scale 2 the R'G'B' entries take odd source sides (mihevc_send_frame_sr_yuv keeps its own even-sides rule).
 * Device memory for the activations is 416 bytes per source pixel at scale 4 and 344 at scale 2 (sr_compact_net.h states the formula).  MIHEVC_EINVAL: NULL
 * model, a scale other than 4 / 2, convs outside 1 .. 64, non-zero reserved, NULL weights, a count other than the model's, slice_count > 1.  MIHEVC_ENOMEM: the
 * device cannot hold the weights; the session has no model then */
int  mihevc_set_sr_compact(mihevc_session *s, const mihevc_sr_compact *model, const float *weights, size_t count);
/* ---- added under ABI 6: a CHAIN of the source filters (symbols only) ----
 * The filters above in series, in one fixed order, every frame of the session through all of them (hevc_amd/csrc/chain_plan.h states the rules):
 *   field        none, the deinterlacer (mihevc_send_frame_deint) or inverse telecine (mihevc_send_frame_fieldmatch)    at the source's size and depth
 *   denoise      off, or the four thresholds of mihevc_send_frame_denoise                                             at the source's size and depth
 *   resize       none, mihevc_send_frame_scaled, mihevc_send_frame_upscaled, or the session's network on the route of   the source's size and depth to the
 *                mihevc_send_frame_sr_yuv (the model of mihevc_set_sr_model / mihevc_set_sr_compact)                    session's
 *   interpolate  off, or mihevc_send_frame_interpolate                                                                at the session's size and depth
 * Every slot is optional and at least one is on.  A stage's picture is the next stage's frame, on the device, with the arithmetic of the single entries: a
 * chain's stream is that of a session fed, through mihevc_send_frame, the pictures the filters' definitions give one after the other.  The source is planar
 * 4:2:0 at 8 or 10 bit with even sides of at least 16, its height a multiple of 4 when the field slot is on; without a resize stage its size and depth are the
 * session's.  Not covered: any other order or a graph of filters, the colour table, format or RGB conversion inside a chain, a resize in front of the field or
 * denoise stage, a chain that changes from frame to frame, sliced sessions and several devices, two stages in one kernel. */
#define MIHEVC_CHAIN_FIELD_NONE  0
#define MIHEVC_CHAIN_FIELD_DEINT 1
#define MIHEVC_CHAIN_FIELD_MATCH 2
#define MIHEVC_CHAIN_RESIZE_NONE    0
#define MIHEVC_CHAIN_RESIZE_SCALE   1
#define MIHEVC_CHAIN_RESIZE_UPSCALE 2
#define MIHEVC_CHAIN_RESIZE_SR      3
typedef struct mihevc_chain {
    int32_t width, height;        /* the source picture: both even, >= 16 */
    int32_t bit_depth;            /* of the source: 8 or 10 */
    int32_t field;                /* MIHEVC_CHAIN_FIELD_* */
    int32_t denoise_on;           /* 0, 1 */
    int32_t resize;               /* MIHEVC_CHAIN_RESIZE_* */
    int32_t interpolate_on;       /* 0, 1 */
    int32_t reserved[9];          /* 0 */
    mihevc_deint deint;                /* field == MIHEVC_CHAIN_FIELD_DEINT */
    mihevc_fieldmatch fieldmatch;      /* field == MIHEVC_CHAIN_FIELD_MATCH */
    mihevc_denoise denoise;            /* denoise_on */
    mihevc_upscale_src upscale;        /* resize == MIHEVC_CHAIN_RESIZE_UPSCALE: sharpen, antiring; width, height and bit_depth repeat the chain's */
    mihevc_sr_yuv sr;                  /* resize == MIHEVC_CHAIN_RESIZE_SR: matrix, full_range of the source; width, height and bit_depth repeat the chain's */
    mihevc_interpolate interpolate;    /* interpolate_on */
} mihevc_chain;
/* The chain of the session, set once, before the first frame: the descriptor is copied.  Everything is judged before any device call.  MIHEVC_EINVAL, leaving
 * the session usable: NULL, non-zero reserved, a selector out of range, no slot on, a source side odd, below 16 or above 8192, a depth other than 8 / 10 (the
 * session's included), a height that is no multiple of 4 with a field stage, whatever the entry of a stage that is on refuses in its struct, a size or depth other
 * than the session's without a resize stage, a ratio the resize stage's entry refuses, MIHEVC_CHAIN_RESIZE_SR without a model or with a cfg.matrix other than
 * 1 / 5 / 6 / 9, width / height / bit_depth of the embedded upscale or sr struct other than the chain's, odd cfg.width / cfg.height, slice_count > 1.  The
 * embedded structs of slots that are off are not looked at.  MIHEVC_ESTATE: a frame has been sent by any entry, a chain is already set, after flush. */
int  mihevc_set_source_chain(mihevc_session *s, const mihevc_chain *chain);
/* A frame of the chain's source size and depth through the chain.  pitch_y, pitch_c: in elements.  Flags, ownership and staging are those of
 * mihevc_send_frame_deint: the frame is copied into the first stage's ring (a chain that begins with its resize stage: into the staging set) on the upload
 * stream, host planes may be reused on return unless MIHEVC_SRC_ASYNC is set, device planes (MIHEVC_SRC_DEVICE) after mihevc_sync_uploads or mihevc_flush.
 * Pictures are numbered consecutively from the first frame's pts, as decimating inverse telecine numbers them: the caller opens the session at the source's
 * rate times the chain's (field rate x2, decimate x4/5, interpolate x factor).  The pts of later frames must increase and are otherwise ignored.
 * mihevc_stats.frames_in counts pictures; mihevc_get_fieldmatch_info works for a chain with an inverse telecine stage.  Rings, hop pictures and the network's
 * arena are allocated at the first frame, nothing per frame; MIHEVC_ENOMEM when the device cannot hold them, before any picture is taken, and the session goes
 * on.  mihevc_flush drains the stages front to back: the field stage's last frame goes into denoise, denoise's last into resize and interpolate, and the
 * interpolator's last frame gives its j = 0 picture.  MIHEVC_EINVAL, decided before any device call: NULL planes, a pitch smaller than the plane, unknown flag
 * bits, a pts that does not increase.  MIHEVC_ESTATE: no chain set, after flush.  While a chain is set every OTHER entry that sends a frame returns
 * MIHEVC_ESTATE. */
int  mihevc_send_frame_chain(mihevc_session *s, const void *y, const void *u, const void *v, int pitch_y, int pitch_c, int64_t pts, int flags);
/* What chain_plan.h says of a descriptor, without a session or a device: width, height, bit_depth and matrix are the session's cfg fields, sr_scale the scale of
 * the network (0: none).  MIHEVC_EINVAL for a descriptor mihevc_set_source_chain refuses with it; else rate_num / rate_den, the reduced fraction the chain
 * multiplies the source's rate by, stages, the slots that are on, pictures, what `frames` frames give once flushed, and the size and depth of every stage. */
typedef struct mihevc_chain_plan {
    int32_t rate_num, rate_den;
    int32_t stages;
    int32_t reserved;
    int64_t pictures;
    int32_t width[4], height[4], bit_depth[4];   /* by slot (field, denoise, resize, interpolate): what the stage runs at, the resize stage: what it writes; 0: off */
} mihevc_chain_plan;
int  mihevc_chain_plan_for(const mihevc_chain *chain, int width, int height, int bit_depth, int matrix, int sr_scale, int64_t frames, mihevc_chain_plan *out);
/* One access unit (Annex-B NAL units) in session-owned memory, valid until the next receive/close. */
int  mihevc_receive_packet(mihevc_session *s, const uint8_t **data, size_t *size,
                           int64_t *pts, int64_t *dts, int *keyframe);
/* ---- added under ABI 6: packets out in ONE call (symbols only) ----
 * Up to `max` ready access units, in decoding order, as mihevc_receive_packet would hand them out one after the other: data[i], size[i], pts[i], dts[i] and
 * keyframe[i] of the i-th (pts, dts and keyframe may be NULL), for a caller that drains a whole clip at a time — a host language's call overhead (ctypes: ~3.5 us
 * per call and more per by-reference argument) is paid once, not per packet.  Returns the number of packets, at least 1; MIHEVC_EAGAIN when nothing is ready and
 * the session is not flushed, MIHEVC_EOF when it is flushed and drained; MIHEVC_EINVAL: max <= 0, NULL data or size (the session stays usable), or the host coder
 * refused the next picture (the session has failed, as with the one-packet form; packets in front of that picture are handed out first).  Every packet of the
 * call stays valid until the next receive call of either kind, or close; the two calls mix in any order. */
int  mihevc_receive_packets(mihevc_session *s, int max, const uint8_t **data, size_t *size,
                            int64_t *pts, int64_t *dts, int *keyframe);
int  mihevc_flush(mihevc_session *s);                /* no more input; drain with receive_packet until MIHEVC_EOF */
/* Give the session up: it fails every later call, and if it codes one slice of a picture with slice_halo, the sessions of the other slices
 * stop waiting for it (their calls return MIHEVC_EDEVICE).  For a driver whose thread hit an error; mihevc_close is still due. */
int  mihevc_abort(mihevc_session *s);
void mihevc_close(mihevc_session *s);
int  mihevc_get_stats(const mihevc_session *s, mihevc_stats *out);
/* VPS+SPS+PPS (Annex-B) for the muxer's hvcC box; valid until close. */
int  mihevc_get_headers(mihevc_session *s, const uint8_t **data, size_t *size);
/* Copy the reconstruction of output frame `index` (display order) as 16-bit planes of the CODED size; only
 * available when the session was opened with keep_recon (tests): returns MIHEVC_ESTATE otherwise. */
int  mihevc_set_keep_recon(mihevc_session *s, int keep);
int  mihevc_get_recon(mihevc_session *s, int64_t index, uint16_t *y, uint16_t *u, uint16_t *v);
int  mihevc_coded_size(const mihevc_session *s, int *w, int *h);
/* QP, slice type (2 = IDR, 1 = P) and coded size in bits (-1 while CABAC is still running) of output picture `index` */
int  mihevc_get_frame_info(mihevc_session *s, int64_t index, int *qp, int *slice_type, int64_t *bits);
/* Quality of output picture `index` (display order, as mihevc_get_frame_info) over the coded size, per colour component (Y, Cb, Cr): sse = squared error of the
 * final reconstruction against the source (PSNR = 10 log10(peak^2 samples / sse)); with cfg.ssim, ssim_q32 = the int64 sum over the picture's windows of each
 * window's SSIM in units of 2^-32 and ssim_windows = their number ((W/4 - 1)(H/4 - 1) of a W x H plane): SSIM = ssim_q32 / (ssim_windows * 2^32).  Any of the three
 * may be NULL.  MIHEVC_ESTATE: no such picture, or ssim_* asked of a session opened with cfg.ssim = 0; MIHEVC_EAGAIN: the picture's results have not reached the
 * host yet (they come with its packet) */
int  mihevc_get_frame_quality(mihevc_session *s, int64_t index, uint64_t sse[3], int64_t ssim_q32[3], int64_t ssim_windows[3]);
const char *mihevc_strerror(int err);
/* s = NULL: what the calling thread's last mihevc_encode_picture_host refused ("null session" when nothing) */
const char *mihevc_last_error(const mihevc_session *s);

/* ---- integer cost parameters derived from a QP (shared by every stage; exported so tests can hand the same
 *      numbers to the oracle) ---- */
typedef struct mihevc_cost_params {
    int32_t qp, qp_c, bit_depth, lambda_sad_q4, lambda_q4, me_range;
    int32_t tile_cols, tile_rows;     /* intra pictures: uniform tile grid (0/1 = one tile); see mihevc_tile_grid */
    int32_t intra_nxn;                /* 1: try part_mode NxN (four 4x4 PUs, DST-VII) for 8x8 intra CUs */
    int32_t intra_in_p;               /* 1: mihevc_k_inter_frame also runs the intra second pass of P pictures */
    int32_t pre_search;               /* 1: without explicit centres, mihevc_k_inter_frame derives them from the 1/4-size pictures */
    int32_t rdo_zero;                 /* 1: RD zero-out of inter TUs */
    int32_t chroma_modes;             /* 1: chroma intra mode decision (else DM) */
    int32_t mc_top, mc_bottom;        /* 1: motion compensation must not read above row 0 / below the last row (the picture is a slice whose
                                       * neighbour lives on another device); 0: the padded border is the picture's own */
    int32_t rdo_cg;                   /* k > 0: RD zero-out of 4x4 coefficient groups of inter TUs with lambda x k / 2; 0: off */
} mihevc_cost_params;
void mihevc_cost_params_for_qp(int qp, int bit_depth, int me_range, mihevc_cost_params *out);   /* tile grid 1x1, every analysis knob 0 */
/* Tile grid of IDR pictures for this configuration: the most columns/rows Table A.8 allows at cfg->level_idc with every
 * column >= 256 and every row >= 64 luma samples (A.4.1), uniform spacing; 1x1 when cfg->intra_tiles == 0. */
int  mihevc_tile_grid(const mihevc_config *cfg, int *cols, int *rows);
/* the same for P pictures (cfg->p_tiles): 1x1 when off */
int  mihevc_p_tile_grid(const mihevc_config *cfg, int *cols, int *rows);

/* per-8x8-block record produced by the analysis kernels and consumed by deblocking and the host entropy coder */
typedef struct mihevc_cu_rec {
    uint8_t log2_size;     /* CU size 3..5 (CU = PU = TU except intra NxN) */
    uint8_t flags;         /* bit0 inter, bit1 cbf_y, bit2 cbf_cb, bit3 cbf_cr, bit4 intra NxN; inter CUs of B pictures: bit5 list 1 is used (its vector: two
                            * little-endian int16 in intra_mode[0..3], which inter CUs do not use), bit6 list 0 is NOT used; neither: list 0 only (P pictures) */
    uint8_t chroma_mode;   /* chroma intra prediction mode 0..34 */
    uint8_t qp;
    uint8_t intra_mode[4];
    int16_t mvx, mvy;      /* quarter-sample units */
    uint8_t cbf_y4;
    uint8_t pad[3];
} mihevc_cu_rec;

typedef struct mihevc_sao_ctu {
    uint8_t type[2];       /* luma, chroma: 0 off, 1 band, 2 edge */
    uint8_t eo_class[2];
    uint8_t band_pos[3];
    int8_t  offset[3][4];
    uint8_t pad;
} mihevc_sao_ctu;

/* ---- per-stage entry points: host buffers in, host buffers out, one device pass each.  They run the SAME kernels
 *      the session runs, so the parity tests (tests/test_gpu_parity.py) hit each stage alone.  Sample planes are
 *      uint8_t when bit_depth == 8 and uint16_t otherwise; pitches are in samples. ---- */
/* K3: forward transform + quantisation + dequantisation + inverse transform of n_blocks residual blocks; log2n 2..5 (4/8/16/32-point
 * DCT); dst4 = 1 with log2n = 2 selects the 4x4 DST-VII of intra luma TUs (8.6.4.2) */
int mihevc_k_transform(int device, const int16_t *residual, int16_t *levels, int16_t *recon_residual,
                       int n_blocks, int log2n, int qp, int bit_depth, int intra, int dst4);
/* the same with sign data hiding (mihevc_config.sign_hide): sign_hide = 1 brings every 4x4 group of every block to the parity rule, scan_idx (0 diagonal,
 * 1 horizontal, 2 vertical: 7.4.9.11) being the block's scan order.  sign_hide = 0 and scan_idx = 0: exactly mihevc_k_transform */
int mihevc_k_transform_sdh(int device, const int16_t *residual, int16_t *levels, int16_t *recon_residual,
                           int n_blocks, int log2n, int qp, int bit_depth, int intra, int dst4, int scan_idx, int sign_hide);
/* K2+K3: intra picture analysis -> pre-deblock reconstruction, CU records, levels */
int mihevc_k_intra_frame(int device, const void *src_y, const void *src_u, const void *src_v, int width, int height,
                         const mihevc_cost_params *prm, void *rec_y, void *rec_u, void *rec_v,
                         mihevc_cu_rec *cu, int16_t *coef_y, int16_t *coef_u, int16_t *coef_v,
                         uint64_t *est_bits_q4 /* optional: the picture's rate estimate in 1/16 bit (rate control input) */);
/* added under ABI 6 (symbols only).  Stage A of mihevc_k_intra_frame alone: the intra PLAN of every CTU (raster order), as the plan kernel leaves it in
 * device memory for the code stage — 64 bytes per CTU.  Index = quadtree node: 0 the 32x32, 1..4 the 16x16 in z-order, 5..20 the 8x8 (the four of 16x16
 * number 1 first, each group in z-order).  chosen[n] = 1: node n is a leaf (a CU) of the planned tree; mode[n] / cmode[n]: the luma / chroma intra
 * prediction mode planned for node n, 0..34, decided for EVERY node that lies wholly inside the picture, chosen or not.  A node that does not: chosen 0,
 * and mode / cmode carry nothing (the kernel never writes them); this entry returns them and `pad` as 0.  DESIGN.md §6 has the rules.  prm as for
 * mihevc_k_intra_frame (qp, qp_c, bit_depth, lambda_sad_q4, lambda_q4, tile_cols / tile_rows, chroma_modes are read); a tile grid with more columns /
 * rows than the picture has CTUs: MIHEVC_EINVAL */
typedef struct mihevc_intra_plan {
    uint8_t chosen[21], mode[21], cmode[21], pad;
} mihevc_intra_plan;
int mihevc_k_intra_plan(int device, const void *src_y, const void *src_u, const void *src_v, int width, int height,
                        const mihevc_cost_params *prm, mihevc_intra_plan *plan_out);
/* K1+K3: inter picture analysis against one (unpadded) reference reconstruction */
int mihevc_k_inter_frame(int device, const void *src_y, const void *src_u, const void *src_v,
                         const void *ref_y, const void *ref_u, const void *ref_v, int width, int height,
                         const mihevc_cost_params *prm, const int16_t *centers, void *rec_y, void *rec_u, void *rec_v,
                         mihevc_cu_rec *cu, int16_t *coef_y, int16_t *coef_u, int16_t *coef_v, int32_t *me_dump,
                         uint64_t *est_bits_q4);
/* K1+K3 for a B picture (cfg.bframes) between two anchors: ref0 = the (unpadded) reconstruction of the anchor before it in display order (list 0), ref1 = the
 * anchor after it (list 1); both integer searches, list-0 tree, list-1 refinement, bi-prediction trial.  centers0 / centers1, me_dump0 / me_dump1: per list */
int mihevc_k_b_frame(int device, const void *src_y, const void *src_u, const void *src_v,
                     const void *ref0_y, const void *ref0_u, const void *ref0_v, const void *ref1_y, const void *ref1_u, const void *ref1_v, int width, int height,
                     const mihevc_cost_params *prm, const int16_t *centers0, const int16_t *centers1, void *rec_y, void *rec_u, void *rec_v,
                     mihevc_cu_rec *cu, int16_t *coef_y, int16_t *coef_u, int16_t *coef_v, int32_t *me_dump0, int32_t *me_dump1, uint64_t *est_bits_q4);
/* K4a: deblocking in place (the picture passes: a session runs them only without SAO, see mihevc_k_loop_filter) */
int mihevc_k_deblock(int device, void *rec_y, void *rec_u, void *rec_v, int width, int height,
                     const mihevc_cu_rec *cu, int bit_depth);
/* K4b: SAO statistics + decision + apply */
int mihevc_k_sao(int device, const void *src_y, const void *src_u, const void *src_v,
                 const void *dbk_y, const void *dbk_u, const void *dbk_v, int width, int height,
                 const mihevc_cost_params *prm, void *out_y, void *out_u, void *out_v, mihevc_sao_ctu *sao);
/* K4 in one pass (what a session runs): the CTU programs deblock their own tile of the PRE-deblock reconstruction `rec_*` (halo of 4 luma / 2 chroma samples),
 * then decide and apply SAO.  Result = mihevc_k_deblock followed by mihevc_k_sao, bit for bit. */
int mihevc_k_loop_filter(int device, const void *src_y, const void *src_u, const void *src_v,
                         const void *rec_y, const void *rec_u, const void *rec_v, int width, int height, const mihevc_cu_rec *cu,
                         const mihevc_cost_params *prm, void *out_y, void *out_u, void *out_v, mihevc_sao_ctu *sao);

/* Decoded picture hash (H.265 Annex D, SEI payloadType 132) of one picture, host planes as above (width x height luma, chroma 4:2:0; coded sizes:
 * multiples of 8): hash_type 0 MD5 (on the host; no device needed), 1 CRC, 2 checksum (the session's kernels).  out: hash_type 0 three 16-byte digests
 * (Y, Cb, Cr), else three uint32_t (a CRC in the low 16 bits) */
int mihevc_k_picture_hash(int device, const void *y, const void *u, const void *v, int width, int height, int bit_depth, int hash_type, void *out);

/* SSIM (mihevc_config.ssim) of one picture pair, host planes as above: a = source, b = reconstruction.  The session's kernels.  sum_q32[c] / (windows[c] * 2^32) is
 * the SSIM of component c */
int mihevc_k_ssim(int device, const void *a_y, const void *a_u, const void *a_v, const void *b_y, const void *b_u, const void *b_v,
                  int width, int height, int bit_depth, int64_t sum_q32[3], int64_t windows[3]);

/* added under ABI 6.  The conversion of mihevc_send_frame_fmt alone (the session's kernel), host buffers in and out: width x height is the display size (both
 * even), out_* are planes of the CODED size (rounded up to 8; chroma half of it each way) with pitch = coded width, uint8_t when out_bit_depth == 8 and
 * uint16_t when 10.  Arguments are validated first (MIHEVC_EINVAL), then MIHEVC_ENODEV without a device */
int mihevc_k_convert_source(int device, const mihevc_src_format *fmt, const void *y, const void *u, const void *v,
                            int width, int height, int pitch_y, int pitch_c, int out_bit_depth,
                            void *out_y, void *out_u, void *out_v);
/* added under ABI 6.  The conversion of mihevc_send_frame_rgb alone (the session's kernel), host buffers in and out; sizes and output planes as
 * mihevc_k_convert_source.  There is no session to follow: fmt->matrix must be 1 / 5 / 6 / 9 and fmt->range 1 or 2.  Validated first (MIHEVC_EINVAL), then
 * MIHEVC_ENODEV without a device */
int mihevc_k_convert_rgb(int device, const mihevc_rgb_format *fmt, const void *p0, const void *p1, const void *p2,
                         int width, int height, int pitch, int out_bit_depth, void *out_y, void *out_u, void *out_v);
/* added under ABI 6.  The kernel of mihevc_send_frame_lut3d alone (the session's kernel), host buffers in and out: table as mihevc_set_lut3d takes it; sizes as
 * mihevc_k_convert_source; out[c] are planes of the CODED size with out_stride[c] samples per row (>= the coded width of the plane), uint8_t when out_bit_depth
 * == 8 and uint16_t when 10.  There is no session to follow: out_matrix must be 1 / 5 / 6 / 9, out_full_range 0 or 1.  Validated first (MIHEVC_EINVAL: what
 * mihevc_send_frame_lut3d and mihevc_set_lut3d refuse, a NULL table or output, a short stride), then MIHEVC_ENODEV without a device */
int mihevc_k_lut3d(int device, const mihevc_lut3d_src *src, int n, const uint16_t *table, const void *y, const void *u, const void *v,
                   int pitch_y, int pitch_c, int width, int height, int out_bit_depth, int out_matrix, int out_full_range,
                   void *const out[3], const int out_stride[3]);
/* added under ABI 6.  The scaler of mihevc_send_frame_scaled alone (the session's kernel), host buffers in and out: src names the source planes y / u / v,
 * dst_width x dst_height is the display size of the output, out_* are planes of its CODED size as in mihevc_k_convert_source.  Validated first
 * (MIHEVC_EINVAL: what mihevc_send_frame_scaled refuses, an out_bit_depth other than 8 or 10), then MIHEVC_ENODEV without a device */
int mihevc_k_scale_source(int device, const mihevc_scale_src *src, const void *y, const void *u, const void *v, int pitch_y, int pitch_c,
                          int dst_width, int dst_height, int out_bit_depth, void *out_y, void *out_u, void *out_v);
/* added under ABI 6.  The deinterlacer of mihevc_send_frame_deint alone (the session's kernel), host buffers in and out: prev / cur / next name the Y, Cb and Cr
 * planes of three frames of width x height samples at bit_depth (they may name the same planes), one pitch_y and one pitch_c for all of them, in elements; keep:
 * parity of the rows that are kept, second: 1 when that field is the later one of its frame; out_* are planes of the CODED size as in mihevc_k_convert_source.
 * Validated first (MIHEVC_EINVAL: a NULL plane, width odd, height not a multiple of 4, either below 16, a short pitch, a bit_depth other than 8 or 10, keep or
 * second outside {0, 1}), then MIHEVC_ENODEV without a device */
int mihevc_k_deinterlace(int device, const void *const prev[3], const void *const cur[3], const void *const next[3],
                         int width, int height, int pitch_y, int pitch_c, int bit_depth, int keep, int second,
                         void *out_y, void *out_u, void *out_v);

/* added under ABI 6.  The denoiser of mihevc_send_frame_denoise alone (the session's kernel), host buffers in and out: prev / cur / next name the Y, Cb and Cr
 * planes of three frames of width x height samples at bit_depth (they may name the same planes), one pitch_y and one pitch_c for all of them, in elements; out_*
 * are planes of the CODED size as in mihevc_k_convert_source.  Validated first (MIHEVC_EINVAL: what mihevc_send_frame_denoise refuses, a bit_depth other than 8
 * or 10), then MIHEVC_ENODEV without a device */
int mihevc_k_denoise(int device, const mihevc_denoise *d, const void *const prev[3], const void *const cur[3], const void *const next[3],
                     int width, int height, int pitch_y, int pitch_c, int bit_depth, void *out_y, void *out_u, void *out_v);

/* added under ABI 6.  The metrics of mihevc_send_frame_fieldmatch alone (k_fm_metrics and its fold, the session's kernels), host buffers in and out: prev_y /
 * cur_y / next_y name the luma planes of three frames of width x height samples at bit_depth (they may name the same plane), one pitch for all of them, in
 * elements; keep: parity of the rows of the declared first field.  out: S_c S_p S_n K_c K_p K_n DS DB as the kernel takes them (the all-ones of a clip's first
 * frame are the session's).  Validated first (MIHEVC_EINVAL: a NULL pointer, width odd, height not a multiple of 4, either below 16, a short pitch, a bit_depth
 * other than 8 or 10, keep outside {0, 1}), then MIHEVC_ENODEV without a device */
int mihevc_k_fieldmatch_metrics(int device, const void *prev_y, const void *cur_y, const void *next_y, int width, int height, int pitch, int bit_depth, int keep,
                                uint64_t out[8]);
/* added under ABI 6.  The weave of mihevc_send_frame_fieldmatch alone (k_fm_weave, the session's kernel), host buffers in and out: cur / other name the Y, Cb
 * and Cr planes of the frame whose rows of parity keep are taken and of the frame that gives the other rows (they may name the same planes); out_* are planes of
 * the CODED size as in mihevc_k_convert_source.  Validated first (MIHEVC_EINVAL: as mihevc_k_deinterlace), then MIHEVC_ENODEV without a device */
int mihevc_k_fieldmatch_weave(int device, const void *const cur[3], const void *const other[3], int width, int height, int pitch_y, int pitch_c, int bit_depth,
                              int keep, void *out_y, void *out_u, void *out_v);
/* added under ABI 6.  The vector search of mihevc_send_frame_interpolate alone (k_mcfi_search and k_mcfi_field, the session's kernels), host buffers in and out:
 * cur_y / next_y are the luma planes of frames k and k + 1, pitch in elements; v0 and v take ceil(height / 8) x ceil(width / 8) pairs (vx, vy): the field of the
 * search and the final one; *scene_sum takes D.  Validated first (MIHEVC_EINVAL: NULL, width or height odd or below 16 or beyond the session limits, a pitch
 * below width, a bit_depth other than 8 or 10), then MIHEVC_ENODEV without a device */
int mihevc_k_mcfi_vectors(int device, const void *cur_y, const void *next_y, int width, int height, int pitch, int bit_depth, int16_t *v0, int16_t *v,
                          uint64_t *scene_sum);
/* added under ABI 6.  Picture j of mihevc_send_frame_interpolate alone (k_mcfi_render, the session's kernel), host buffers in and out: cur / next name the Y, Cb
 * and Cr planes of frames k and k + 1; v is a field as mihevc_k_mcfi_vectors gives it, but the CALLER's (not read under mode blend, where it may be NULL);
 * scene_sum is D; out_* are planes of the CODED size as in mihevc_k_convert_source.  Validated first (MIHEVC_EINVAL: what mihevc_send_frame_interpolate
 * refuses, j outside 0 .. factor - 1, a component of v outside [-18, 18], a bit_depth other than 8 or 10), then MIHEVC_ENODEV without a device */
int mihevc_k_mcfi_render(int device, const mihevc_interpolate *d, int j, const void *const cur[3], const void *const next[3], const int16_t *v, uint64_t scene_sum,
                         int width, int height, int pitch_y, int pitch_c, int bit_depth, void *out_y, void *out_u, void *out_v);
/* added under ABI 6.  The upscaler of mihevc_send_frame_upscaled alone (k_upscale, the session's kernel), host buffers in and out: src names the source planes
 * y / u / v, dst_width x dst_height is the display size of the output, out_* are planes of its CODED size as in mihevc_k_convert_source.  Validated first
 * (MIHEVC_EINVAL: what mihevc_send_frame_upscaled refuses, an out_bit_depth other than 8 or 10), then MIHEVC_ENODEV without a device */
int mihevc_k_upscale_source(int device, const mihevc_upscale_src *src, const void *y, const void *u, const void *v, int pitch_y, int pitch_c,
                            int dst_width, int dst_height, int out_bit_depth, void *out_y, void *out_u, void *out_v);
/* added under ABI 6.  One launch of k_sr_conv (hevc_amd/csrc/kernels/sr_conv.h), host arrays in and out.  Tensors are IEEE halves, NHWC.  `in`: the source
 * tensor of in_ch channels, width x height pixels, or with up = 1 ((height + 1) / 2) x ((width + 1) / 2); the launch reads cin channels (a multiple of 32, at
 * most 192) from in_off on.  weights: fp32 [cout][cin_real][3][3], packed here (input channels cin_real .. cin - 1 meet zero weights); bias: cout.  `out` is read
 * AND written: it is uploaded as given, the launch writes cout channels (32 or 64) from out_off on of its out_ch, and it comes back whole.  planar = 1: cout is
 * 3, n_res is 0 and out is three planes of height x width.  act: LeakyReLU with `slope`.  n_res 0 .. 2: v = v a1 + r1, then v = v a2 + r2; r1 / r2 are tensors of the
 * output's size with r*_ch channels, read from r*_off on.  Channel counts and offsets of buffers are multiples of 8.  MIHEVC_EINVAL first, then MIHEVC_ENODEV */
typedef struct mihevc_sr_conv_desc {
    int32_t width, height;                           /* of the output */
    int32_t up, planar, act, n_res;
    int32_t in_ch, in_off, cin, cin_real;
    int32_t out_ch, out_off, cout;
    int32_t r1_ch, r1_off, r2_ch, r2_off;
    float slope, a1, a2;
} mihevc_sr_conv_desc;
int mihevc_k_sr_conv(int device, const mihevc_sr_conv_desc *d, const uint16_t *in, const float *weights, const float *bias, const uint16_t *r1, const uint16_t *r2,
                     uint16_t *out);
/* added under ABI 6.  k_sr_input alone: a source as mihevc_send_frame_rgb takes it (fmt->matrix and fmt->range are not used) -> the network's input tensor of 32
 * channels: src_width x src_height pixels at scale 4, half of that each way at scale 2 */
int mihevc_k_sr_input(int device, const mihevc_rgb_format *fmt, int scale, int src_width, int src_height, const void *p0, const void *p1, const void *p2, int pitch,
                      uint16_t *out);
/* added under ABI 6.  The whole network as mihevc_send_frame_sr runs it (k_sr_input, then every launch of sr_net.h), from host arrays: weights / count as
 * mihevc_set_sr_model takes them; out: three planes (R, G, B) of halves, scale x the source size.  MIHEVC_ENOMEM when the device cannot hold the size */
int mihevc_k_sr_network(int device, const mihevc_sr_model *model, const float *weights, size_t count, const mihevc_rgb_format *fmt, int src_width, int src_height,
                        const void *p0, const void *p1, const void *p2, int pitch, uint16_t *out);
/* added under ABI 6.  k_sr_from_yuv alone (the session's kernel): a source as mihevc_send_frame_sr_yuv takes it, host arrays in -> the network's input tensor of
 * 32 channels, the shape mihevc_k_sr_input returns: src->width x src->height pixels at scale 4, half of that each way at scale 2 */
int mihevc_k_sr_from_yuv(int device, const mihevc_sr_yuv *src, int scale, const void *y, const void *u, const void *v, int pitch_y, int pitch_c, uint16_t *out);
/* added under ABI 6.  One launch of k_sr_compact (hevc_amd/csrc/kernels/sr_compact.h), host arrays in and out.  Tensors are IEEE halves, NHWC.  `in`: width x
 * height pixels of cin channels (32 or 64; input channels cin_real .. cin - 1 meet zero weights).  tail = 0: weights fp32 [64][cin_real][3][3], bias [64],
 * slopes [64] (PReLU, one per channel); out: 64 channels.  tail = 1 (cin 64, scale 4 or 2): weights [3 r r][cin_real][3][3], bias [3 r r], slopes not read; base:
 * the input tensor of the network, width x height pixels of 32 channels, of which channels 0 .. 2 are added; out: three planes of (r height) x (r width).  `out`
 * is uploaded as given and comes back whole.  MIHEVC_EINVAL first (a NULL array the launch reads, a side below 1 or above 8192, another cin, cin_real outside
 * 1 .. cin, tail outside {0, 1}, with tail another scale or cin, non-zero reserved), then MIHEVC_ENODEV */
typedef struct mihevc_sr_compact_conv_desc {
    int32_t width, height;
    int32_t cin, cin_real;
    int32_t tail, scale;     /* scale: read with tail = 1 */
    int32_t reserved[2];     /* 0 */
} mihevc_sr_compact_conv_desc;
int mihevc_k_sr_compact_conv(int device, const mihevc_sr_compact_conv_desc *d, const uint16_t *in, const float *weights, const float *bias, const float *slopes,
                             const uint16_t *base, uint16_t *out);
/* added under ABI 6.  The whole compact network as mihevc_send_frame_sr runs it (k_sr_input, then every launch of sr_compact_net.h), from host arrays: weights /
 * count as mihevc_set_sr_compact takes them; out: three planes (R, G, B) of halves, scale x the source size.  Sides of at least 4, odd ones included.
 * MIHEVC_ENOMEM when the device cannot hold the size */
int mihevc_k_sr_compact_network(int device, const mihevc_sr_compact *model, const float *weights, size_t count, const mihevc_rgb_format *fmt, int src_width,
                                int src_height, const void *p0, const void *p1, const void *p2, int pitch, uint16_t *out);

/* added under ABI 6 (symbols only).  The scene-cut detector of a session alone (mihevc_config.scenecut; the session's kernel and launcher, on zeroed sums): luma[i] is
 * the luma plane of picture i in host memory, pitch[i] x height samples (pitch[i] >= width, in samples; uint8_t at bit_depth 8, uint16_t at 10), width and height
 * at least 1.  out[i], i >= 1: the sum of |luma[i - 1][y][x] - luma[i][y][x]| over every 4th sample of every 4th row (x, y = 0 mod 4) inside width x height;
 * out[0] = 0.  n = 1 is allowed and gives out[0] = 0.  Refused before anything is launched (MIHEVC_EINVAL): n < 1, a null plane, a pitch below width, a bit depth
 * other than 8 / 10; then MIHEVC_ENODEV without a device */
int mihevc_k_scene_diff(int device, const void *const *luma, const int32_t *pitch /* samples */, int n, int width, int height, int bit_depth,
                        uint64_t *out /* n; out[0] = 0 */);

/* ---- host-only stages (no device needed): bitstream ---- */
/* VPS+SPS+PPS (+SEI when hdr10) as Annex-B into buf; returns size or negative error */
int mihevc_write_parameter_sets(const mihevc_config *cfg, uint8_t *buf, size_t cap);
/* The decoded picture hash suffix SEI NAL unit (Annex-B, type 40, payloadType 132) into buf: hash_type 0 MD5, 1 CRC, 2 checksum; values as the
 * out of mihevc_k_picture_hash.  Returns size or negative error */
int mihevc_write_picture_hash_sei(const mihevc_config *cfg, int hash_type, const void *values, uint8_t *buf, size_t cap);
/* CABAC-code one picture from its symbols into one slice NAL (+AUD when cfg->aud); returns size or negative error.
 * slice_type 2 = I (IDR), 1 = P, 0 = B (cfg->bframes); poc = position inside the closed GOP in display order. */
int mihevc_encode_picture_host(const mihevc_config *cfg, int slice_type, int poc, int qp,
                               const mihevc_cu_rec *cu, const int16_t *coef_y, const int16_t *coef_u, const int16_t *coef_v,
                               const mihevc_sao_ctu *sao, uint8_t *buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* MIHEVC_H */
