"""ctypes binding of hevc_amd/libmihevc.so (C ABI: include/mihevc.h).

The library holds the gfx950 code objects, the host CABAC/bitstream writer and the session pipeline.  There is no
Python or CPU fallback for any of it: `load()` raises if the shared object is missing or an exported symbol the
header declares is absent, and every encode entry point returns MIHEVC_ENODEV on a host without an MI355X.
"""
from __future__ import annotations

import ctypes as C
import numbers
import os
from pathlib import Path

HERE = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("MIHEVC_LIBRARY", HERE / "libmihevc.so"))      # override: A/B runs of two builds in one GPU call

OK, EAGAIN, EOF, EINVAL, ENODEV, ENOMEM, EDEVICE, ESTATE = 0, -1, -2, -3, -4, -5, -6, -7


class Config(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in (
        "width", "height", "fps_num", "fps_den", "bit_depth", "level_idc", "tier", "crf", "qp", "vbv_maxrate_kbps",
        "vbv_bufsize_kbits", "keyint", "min_keyint", "colour_primaries", "transfer", "matrix", "full_range", "chroma_loc",
        "aud", "repeat_headers", "hdr10")] +
        [("md_primaries", (C.c_uint16 * 2) * 3), ("md_white", C.c_uint16 * 2), ("md_max_lum", C.c_uint32), ("md_min_lum", C.c_uint32),
         ("max_cll", C.c_uint16), ("max_fall", C.c_uint16)] +
        [(n, C.c_int32) for n in ("me_range", "gops_in_flight", "host_threads", "sao", "profile_stages", "intra_tiles", "intra_nxn", "intra_in_p", "hrd", "pre_search", "rdo_zero", "chroma_modes", "pic_height", "slice_count", "slice_index")] +
        [("slice_ctu_rows", C.c_int32 * 16), ("rate_share_q16", C.c_int32), ("scenecut", C.c_int32), ("gop_balance", C.c_int32), ("rdo_cg", C.c_int32), ("p_tiles", C.c_int32), ("bframes", C.c_int32), ("b_qp_offset", C.c_int32), ("slice_halo", C.c_int32), ("slice_group", C.c_int32), ("sign_hide", C.c_int32), ("pic_hash", C.c_int32), ("ssim", C.c_int32)])


class Stats(C.Structure):
    _fields_ = [("frames_in", C.c_int64), ("frames_out", C.c_int64), ("bytes_out", C.c_int64), ("sse_y", C.c_double), ("sse_u", C.c_double),
                ("sse_v", C.c_double), ("device_ms", C.c_double), ("entropy_ms", C.c_double), ("last_qp", C.c_int32), ("reserved", C.c_int32 * 7),
                ("stage_ms", C.c_double * 8), ("stage_launches", C.c_int64 * 8), ("stage_pictures", C.c_int64 * 8),
                ("ssim_y", C.c_double), ("ssim_u", C.c_double), ("ssim_v", C.c_double)]


STAGE_NAMES = ("intra", "me_search", "inter_ctu", "deblock", "sao", "pad", "sse", "intra_p")


class CostParams(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("qp", "qp_c", "bit_depth", "lambda_sad_q4", "lambda_q4", "me_range", "tile_cols", "tile_rows", "intra_nxn", "intra_in_p", "pre_search", "rdo_zero", "chroma_modes", "mc_top", "mc_bottom", "rdo_cg")]


class SrcFormat(C.Structure):
    """mihevc_src_format: the sample layout of a source handed to mihevc_send_frame_fmt / mihevc_k_convert_source"""
    _fields_ = [(n, C.c_int32) for n in ("chroma", "semi_planar", "bit_depth", "msb_aligned")] + [("reserved", C.c_int32 * 4)]

    def __eq__(self, other):
        return isinstance(other, SrcFormat) and bytes(self) == bytes(other)

    __hash__ = None

    def __repr__(self):
        return f"SrcFormat(chroma={self.chroma}, semi_planar={self.semi_planar}, bit_depth={self.bit_depth}, msb_aligned={self.msb_aligned})"

    def chroma_shape(self, width: int, height: int):
        """(rows, elements per row) of a source chroma plane; a semi-planar one holds Cb and Cr side by side"""
        return (height // 2 if self.chroma == 420 else height), (width if self.chroma == 444 else width // 2) * (2 if self.semi_planar else 1)

    def frame_bytes(self, width: int, height: int) -> int:
        rows, row = self.chroma_shape(width, height)
        return (width * height + rows * row * (1 if self.semi_planar else 2)) * (2 if self.bit_depth > 8 else 1)


SRC_DEVICE, SRC_ASYNC = 1, 2

_SEMI_PLANAR = {"nv12": (420, 8), "nv16": (422, 8), "nv24": (444, 8), "p010le": (420, 10), "p016le": (420, 16), "p210le": (422, 10), "p216le": (422, 16),
                "p410le": (444, 10), "p416le": (444, 16)}


def src_format_for(pix_fmt: str):
    """The SrcFormat of an ffmpeg pixel format name, or None for one the conversion does not cover (swapped semi-planar, packed, RGB, 4:1:1 / 4:1:0,
    big endian, alpha).  yuvj* are the same layouts as yuv*: there is no range conversion."""
    import re
    name = (pix_fmt or "").lower()
    if name in _SEMI_PLANAR:
        chroma, depth = _SEMI_PLANAR[name]
        return SrcFormat(chroma, 1, depth, 1 if depth > 8 else 0)
    m = re.fullmatch(r"yuvj?(420|422|444)p(?:(9|10|12|14|16)le)?", name)
    if not m or (m.group(2) and name.startswith("yuvj")):
        return None
    return SrcFormat(int(m.group(1)), 0, int(m.group(2) or 8), 0)


class ScaleSrc(C.Structure):
    """mihevc_scale_src: size and depth of a planar 4:2:0 source handed to mihevc_send_frame_scaled / mihevc_k_scale_source"""
    _fields_ = [(n, C.c_int32) for n in ("width", "height", "bit_depth")] + [("reserved", C.c_int32 * 5)]

    def __repr__(self):
        return f"ScaleSrc(width={self.width}, height={self.height}, bit_depth={self.bit_depth})"


class Deint(C.Structure):
    """mihevc_deint: field order and output rate of the interlaced frames handed to mihevc_send_frame_deint"""
    _fields_ = [(n, C.c_int32) for n in ("tff", "field_rate")] + [("reserved", C.c_int32 * 6)]

    def __repr__(self):
        return f"Deint(tff={self.tff}, field_rate={self.field_rate})"


class Fieldmatch(C.Structure):
    """mihevc_fieldmatch: declared field order and what inverse telecine does with the frames handed to mihevc_send_frame_fieldmatch"""
    _fields_ = [(n, C.c_int32) for n in ("tff", "decimate", "deint")] + [("reserved", C.c_int32 * 5)]

    def __repr__(self):
        return f"Fieldmatch(tff={self.tff}, decimate={self.decimate}, deint={self.deint})"


class FmFrame(C.Structure):
    """mihevc_fm_frame: what mihevc_get_fieldmatch_info tells about one frame: the metrics (c, p, n), the match, and where the picture went"""
    _fields_ = [("comb_sum", C.c_uint64 * 3), ("comb_block", C.c_uint32 * 3), ("dup_sum", C.c_uint64), ("dup_block", C.c_uint32), ("match", C.c_int32),
                ("deinterlaced", C.c_int32), ("dropped", C.c_int32), ("picture", C.c_int64)]


class Denoise(C.Structure):
    """mihevc_denoise: the four thresholds, in 8-bit units, of the frames handed to mihevc_send_frame_denoise / mihevc_k_denoise"""
    _fields_ = [(n, C.c_int32) for n in ("luma_spatial", "luma_temporal", "chroma_spatial", "chroma_temporal")] + [("reserved", C.c_int32 * 4)]

    def __repr__(self):
        return f"Denoise({self.luma_spatial}, {self.luma_temporal}, {self.chroma_spatial}, {self.chroma_temporal})"


# denoise level -> (luma_spatial, luma_temporal, chroma_spatial, chroma_temporal); level 0: the filter is the identity (DESIGN.md §6g has the tables behind them)
DENOISE_LEVELS = ((0, 0, 0, 0), (3, 4, 3, 4), (5, 7, 5, 7), (8, 11, 8, 11))


def denoise_level(n: int) -> Denoise:
    """the preset of level n in 0 .. 3"""
    if isinstance(n, bool) or not isinstance(n, int) or not 0 <= n < len(DENOISE_LEVELS):
        raise ValueError(f"denoise level {n!r}: 0 .. {len(DENOISE_LEVELS) - 1}")
    return Denoise(*DENOISE_LEVELS[n])


def denoise_strength(s) -> Denoise:
    """a level 0 .. 3, or four thresholds 0 .. 255 (luma_spatial, luma_temporal, chroma_spatial, chroma_temporal)"""
    if isinstance(s, int):
        return denoise_level(s)
    t = () if isinstance(s, (str, bytes)) else tuple(s)
    if len(t) != 4 or any(isinstance(v, bool) or not isinstance(v, numbers.Integral) or not 0 <= v <= 255 for v in t):
        raise ValueError(f"denoise strength {s!r}: a level 0 .. 3 or four thresholds 0 .. 255")
    return Denoise(*(int(v) for v in t))


class Interpolate(C.Structure):
    """mihevc_interpolate: factor (2, 3 or 4 pictures per frame), mode (0 motion compensated, 1 blend) and scene threshold (0 .. 255 in 8-bit units, 0 off) of the
    frames handed to mihevc_send_frame_interpolate / mihevc_k_mcfi_render"""
    _fields_ = [(n, C.c_int32) for n in ("factor", "mode", "scene_threshold")] + [("reserved", C.c_int32 * 5)]

    def __repr__(self):
        return f"Interpolate(factor={self.factor}, mode={self.mode}, scene_threshold={self.scene_threshold})"


INTERP_MODES = {"mc": 0, "blend": 1}


def interpolate_mode(factor, mode="mc", scene_threshold: int = 10) -> Interpolate:
    """factor 2 .. 4, mode 'mc' or 'blend', scene_threshold 0 .. 255"""
    if isinstance(factor, bool) or not isinstance(factor, int) or not 2 <= factor <= 4:
        raise ValueError(f"interpolate factor {factor!r}: 2, 3 or 4")
    if mode not in INTERP_MODES:
        raise ValueError(f"interpolate mode {mode!r}: 'mc' or 'blend'")
    if isinstance(scene_threshold, bool) or not isinstance(scene_threshold, int) or not 0 <= scene_threshold <= 255:
        raise ValueError(f"scene_threshold {scene_threshold!r}: 0 .. 255")
    return Interpolate(factor, INTERP_MODES[mode], scene_threshold)


class Lut3dSrc(C.Structure):
    """mihevc_lut3d_src: depth, matrix and range of the planar 4:2:0 frames handed to mihevc_send_frame_lut3d / mihevc_k_lut3d"""
    _fields_ = [(n, C.c_int32) for n in ("bit_depth", "matrix", "full_range")] + [("reserved", C.c_int32 * 4)]

    def __repr__(self):
        return f"Lut3dSrc(bit_depth={self.bit_depth}, matrix={self.matrix}, full_range={self.full_range})"


class UpscaleSrc(C.Structure):
    """mihevc_upscale_src: size, depth, sharpening gain (sixteenths, 0 .. 64) and anti-ringing strength (eighths, 0 .. 8) of a planar 4:2:0 source handed to
    mihevc_send_frame_upscaled / mihevc_k_upscale_source"""
    _fields_ = [(n, C.c_int32) for n in ("width", "height", "bit_depth", "sharpen", "antiring")] + [("reserved", C.c_int32 * 3)]

    def __repr__(self):
        return f"UpscaleSrc(width={self.width}, height={self.height}, bit_depth={self.bit_depth}, sharpen={self.sharpen}, antiring={self.antiring})"


class SrModel(C.Structure):
    """mihevc_sr_model: scale (4 or 2) and number of RRDBs of the RRDBNet whose flat weights go with it (hevc_amd.sr.load_rrdbnet)"""
    _fields_ = [("scale", C.c_int32), ("blocks", C.c_int32), ("reserved", C.c_int32 * 6)]

    def __repr__(self):
        return f"SrModel(scale={self.scale}, blocks={self.blocks})"


class SrCompact(C.Structure):
    """mihevc_sr_compact: scale (4 or 2) and number of trunk convolutions of the SRVGGNetCompact whose flat weights go with it (hevc_amd.sr.load_compact)"""
    _fields_ = [("scale", C.c_int32), ("convs", C.c_int32), ("reserved", C.c_int32 * 6)]

    def __repr__(self):
        return f"SrCompact(scale={self.scale}, convs={self.convs})"


class SrCompactConvDesc(C.Structure):
    """mihevc_sr_compact_conv_desc: one launch of k_sr_compact as mihevc_k_sr_compact_conv takes it"""
    _fields_ = [(n, C.c_int32) for n in ("width", "height", "cin", "cin_real", "tail", "scale")] + [("reserved", C.c_int32 * 2)]


class SrYuv(C.Structure):
    """mihevc_sr_yuv: size, depth, matrix and range of the planar 4:2:0 Y'CbCr frames handed to mihevc_send_frame_sr_yuv / mihevc_k_sr_from_yuv"""
    _fields_ = [(n, C.c_int32) for n in ("width", "height", "bit_depth", "matrix", "full_range")] + [("reserved", C.c_int32 * 3)]

    def __repr__(self):
        return f"SrYuv(width={self.width}, height={self.height}, bit_depth={self.bit_depth}, matrix={self.matrix}, full_range={self.full_range})"


CHAIN_FIELD = {None: 0, "deint": 1, "fieldmatch": 2}
CHAIN_RESIZE = {None: 0, "scale": 1, "upscale": 2, "sr": 3}


class Chain(C.Structure):
    """mihevc_chain: the source filter chain of a session (mihevc_set_source_chain): the source's size and depth, one selector per slot (field:
    CHAIN_FIELD, denoise_on, resize: CHAIN_RESIZE, interpolate_on) and the parameter structs of the single entries; chain() fills one in"""
    _fields_ = ([(n, C.c_int32) for n in ("width", "height", "bit_depth", "field", "denoise_on", "resize", "interpolate_on")] + [("reserved", C.c_int32 * 9)] +
                [("deint", Deint), ("fieldmatch", Fieldmatch), ("denoise", Denoise), ("upscale", UpscaleSrc), ("sr", SrYuv), ("interpolate", Interpolate)])

    def __repr__(self):
        return (f"Chain({self.width}x{self.height}@{self.bit_depth}, field={self.field}, denoise={self.denoise_on}, resize={self.resize}, "
                f"interpolate={self.interpolate_on})")


class ChainPlan(C.Structure):
    """mihevc_chain_plan: what mihevc_chain_plan_for says of a chain: the rate fraction, the slots that are on, the pictures of `frames` frames, and by slot
    (field, denoise, resize, interpolate) the size and depth the stage runs at (the resize stage: what it writes; 0: off)"""
    _fields_ = [("rate_num", C.c_int32), ("rate_den", C.c_int32), ("stages", C.c_int32), ("reserved", C.c_int32), ("pictures", C.c_int64), ("width", C.c_int32 * 4),
                ("height", C.c_int32 * 4), ("bit_depth", C.c_int32 * 4)]


def chain(width, height, bit_depth, field=None, tff=True, field_rate=False, decimate=True, fm_deint=True, denoise=None, resize=None, sharpen=8, antiring=8,
          sr_matrix=6, sr_full_range=False, interpolate=None, interp_mode="mc", scene_threshold=10) -> Chain:
    """A Chain for a width x height source at bit_depth.  field: None, 'deint' (tff, field_rate) or 'fieldmatch' (tff, decimate, fm_deint); denoise: None, or what
    denoise_strength takes; resize: None, 'scale', 'upscale' (sharpen, antiring) or 'sr' (sr_matrix, sr_full_range of the source); interpolate: None, or a
    factor 2 .. 4 (interp_mode, scene_threshold).  The ranges are judged by the library (mihevc_set_source_chain, mihevc_chain_plan_for); names and types here"""
    if field not in CHAIN_FIELD or resize not in CHAIN_RESIZE:
        raise ValueError(f"chain: field={field!r} takes None, 'deint' or 'fieldmatch'; resize={resize!r} takes None, 'scale', 'upscale' or 'sr'")
    c = Chain(int(width), int(height), int(bit_depth), CHAIN_FIELD[field], int(denoise is not None), CHAIN_RESIZE[resize], int(interpolate is not None))
    if field == "deint":
        c.deint = Deint(int(bool(tff)), int(bool(field_rate)))
    elif field == "fieldmatch":
        c.fieldmatch = Fieldmatch(int(bool(tff)), int(bool(decimate)), int(bool(fm_deint)))
    if denoise is not None:
        c.denoise = denoise if isinstance(denoise, Denoise) else denoise_strength(denoise)
    if resize == "upscale":
        c.upscale = UpscaleSrc(c.width, c.height, c.bit_depth, int(sharpen), int(antiring))
    elif resize == "sr":
        c.sr = SrYuv(c.width, c.height, c.bit_depth, int(sr_matrix), 1 if sr_full_range else 0)
    if interpolate is not None:
        c.interpolate = interpolate_mode(interpolate, interp_mode, scene_threshold)
    return c


def chain_plan(c: Chain, width: int, height: int, bit_depth: int, matrix: int = 1, sr_scale: int = 0, frames: int = 0):
    """mihevc_chain_plan_for: the ChainPlan of chain c in front of a width x height session at bit_depth (matrix: its cfg.matrix; sr_scale: the scale of its
    network, 0 without one), or None for a descriptor the library refuses"""
    out = ChainPlan()
    rc = load().mihevc_chain_plan_for(C.byref(c), int(width), int(height), int(bit_depth), int(matrix), int(sr_scale), int(frames), C.byref(out))
    return out if rc == 0 else None


class SrConvDesc(C.Structure):
    """mihevc_sr_conv_desc: one launch of k_sr_conv as mihevc_k_sr_conv takes it"""
    _fields_ = ([(n, C.c_int32) for n in ("width", "height", "up", "planar", "act", "n_res", "in_ch", "in_off", "cin", "cin_real", "out_ch", "out_off", "cout",
                                          "r1_ch", "r1_off", "r2_ch", "r2_off")] + [(n, C.c_float) for n in ("slope", "a1", "a2")])


class RgbFormat(C.Structure):
    """mihevc_rgb_format: the sample layout of an RGB source handed to mihevc_send_frame_rgb / mihevc_k_convert_rgb"""
    _fields_ = [(n, C.c_int32) for n in ("layout", "r", "g", "b", "sample", "bit_depth", "matrix", "range")] + [("reserved", C.c_int32 * 4)]

    def __eq__(self, other):
        return isinstance(other, RgbFormat) and bytes(self) == bytes(other)

    __hash__ = None

    def __repr__(self):
        return (f"RgbFormat(layout={self.layout}, r={self.r}, g={self.g}, b={self.b}, sample={self.sample}, bit_depth={self.bit_depth}, matrix={self.matrix}, "
                f"range={self.range})")

    @property
    def element_size(self) -> int:
        return 4 if self.sample == 2 else 2 if self.sample == 1 or self.bit_depth > 8 else 1

    def plane_shapes(self, width: int, height: int):
        """the shapes of the source planes: three (height, width) planes, or one packed (height, layout * width) plane"""
        return [(height, width)] * 3 if self.layout == 0 else [(height, self.layout * width)]

    def frame_bytes(self, width: int, height: int) -> int:
        return width * height * (self.layout or 3) * self.element_size


_PACKED_RGB = {"rgb": (0, 1, 2), "bgr": (2, 1, 0)}


def rgb_format_for(pix_fmt: str, matrix: int = 0, range: int = 0):
    """The RgbFormat of an ffmpeg pixel format name, or None for one the RGB conversion does not cover (big endian, alpha planes, rgb565*, x2rgb10le, pal8,
    gray*, and every Y'CbCr name: those are src_format_for's).  matrix / range: the struct's fields, 0 to follow the session"""
    import re
    name = (pix_fmt or "").lower()
    m = re.fullmatch(r"gbrp(?:(9|10|12|14|16)le|(f32le))?", name)
    if m:       # planes in G, B, R order
        return RgbFormat(0, 2, 0, 1, 2 if m.group(2) else 0, 0 if m.group(2) else int(m.group(1) or 8), matrix, range)
    m = re.fullmatch(r"(rgb|bgr)(24|48le)", name)
    if m:
        return RgbFormat(3, *_PACKED_RGB[m.group(1)], 0, 8 if m.group(2) == "24" else 16, matrix, range)
    m = re.fullmatch(r"(rgb|bgr)(?:[a0]|(a64le))", name)
    if m:
        return RgbFormat(4, *_PACKED_RGB[m.group(1)], 0, 16 if m.group(2) else 8, matrix, range)
    m = re.fullmatch(r"[a0](rgb|bgr)", name)
    if m:
        return RgbFormat(4, *(i + 1 for i in _PACKED_RGB[m.group(1)]), 0, 8, matrix, range)
    return None


# every symbol include/mihevc.h declares; tests/test_abi.py checks the header against this list and the .so
EXPORTS = (
    "mihevc_abi_version", "mihevc_device_count", "mihevc_device_numa_node", "mihevc_config_default", "mihevc_open", "mihevc_send_frame", "mihevc_send_frame_async", "mihevc_sync_uploads", "mihevc_send_frame_device", "mihevc_send_frames_device",
    "mihevc_receive_packet", "mihevc_receive_packets", "mihevc_flush", "mihevc_abort", "mihevc_close", "mihevc_get_stats", "mihevc_get_headers", "mihevc_set_keep_recon",
    "mihevc_get_recon", "mihevc_coded_size", "mihevc_get_frame_info", "mihevc_strerror", "mihevc_last_error", "mihevc_cost_params_for_qp", "mihevc_tile_grid", "mihevc_p_tile_grid", "mihevc_k_transform", "mihevc_k_transform_sdh",
    "mihevc_k_intra_frame", "mihevc_k_inter_frame", "mihevc_k_b_frame", "mihevc_k_deblock", "mihevc_k_sao", "mihevc_k_loop_filter", "mihevc_write_parameter_sets",
    "mihevc_encode_picture_host", "mihevc_k_picture_hash", "mihevc_write_picture_hash_sei", "mihevc_get_frame_quality", "mihevc_k_ssim",
    "mihevc_send_frame_fmt", "mihevc_k_convert_source", "mihevc_k_intra_plan", "mihevc_send_frame_rgb", "mihevc_k_convert_rgb",
    "mihevc_send_frame_scaled", "mihevc_k_scale_source", "mihevc_k_scene_diff", "mihevc_send_frame_deint", "mihevc_k_deinterlace",
    "mihevc_send_frame_denoise", "mihevc_k_denoise", "mihevc_send_frame_fieldmatch", "mihevc_get_fieldmatch_info", "mihevc_k_fieldmatch_metrics",
    "mihevc_k_fieldmatch_weave", "mihevc_set_lut3d", "mihevc_send_frame_lut3d", "mihevc_k_lut3d",
    "mihevc_send_frame_interpolate", "mihevc_k_mcfi_vectors", "mihevc_k_mcfi_render",
    "mihevc_send_frame_upscaled", "mihevc_k_upscale_source",
    "mihevc_set_sr_model", "mihevc_send_frame_sr", "mihevc_k_sr_conv", "mihevc_k_sr_input", "mihevc_k_sr_network",
    "mihevc_send_frame_sr_yuv", "mihevc_send_frame_sr_fit", "mihevc_k_sr_from_yuv",
    "mihevc_set_sr_compact", "mihevc_k_sr_compact_conv", "mihevc_k_sr_compact_network",
    "mihevc_set_source_chain", "mihevc_send_frame_chain", "mihevc_chain_plan_for",
)

_lib = None


class MihevcError(RuntimeError):
    def __init__(self, code: int, what: str = ""):
        self.code = code
        msg = strerror(code)
        super().__init__(f"{what}: {msg} ({code})" if what else f"{msg} ({code})")


def load() -> C.CDLL:
    """Load libmihevc.so; raises OSError/AttributeError loudly when it is missing or incomplete."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise OSError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` (hipcc --offload-arch=gfx950)")
    # several sessions in one process (threads of a batch, SlicedEncoder's bands) are 3 HIP streams each, mapped onto the process's hardware queues; streams sharing
    # one serialise.  The queue count is left to the environment: shared machines cap it, and a process may not raise it past that cap.
    lib = C.CDLL(str(LIB_PATH))
    for name in EXPORTS:
        getattr(lib, name)          # AttributeError if the ABI is incomplete
    vp, i32, i64 = C.c_void_p, C.c_int, C.c_int64
    lib.mihevc_strerror.restype = C.c_char_p
    lib.mihevc_last_error.restype = C.c_char_p
    lib.mihevc_last_error.argtypes = [vp]
    lib.mihevc_config_default.argtypes = [C.POINTER(Config)]
    lib.mihevc_config_default.restype = None
    lib.mihevc_open.argtypes = [C.POINTER(Config), i32, C.POINTER(vp)]
    lib.mihevc_send_frame.argtypes = [vp, vp, vp, vp, i32, i32, i64]
    lib.mihevc_send_frame_device.argtypes = [vp, vp, vp, vp, i32, i32, i64]
    lib.mihevc_send_frame_async.argtypes = [vp, vp, vp, vp, i32, i32, i64]
    lib.mihevc_send_frames_device.argtypes = [vp, i32, vp, vp, vp, i32, i32, i64]
    lib.mihevc_sync_uploads.argtypes = [vp]
    lib.mihevc_receive_packet.argtypes = [vp, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_size_t), C.POINTER(i64), C.POINTER(i64), C.POINTER(i32)]
    lib.mihevc_receive_packets.argtypes = [vp, i32, vp, vp, vp, vp, vp]      # arrays of c_void_p, c_size_t, c_int64, c_int64, c_int
    lib.mihevc_flush.argtypes = [vp]
    lib.mihevc_abort.argtypes = [vp]
    lib.mihevc_close.argtypes = [vp]
    lib.mihevc_close.restype = None
    lib.mihevc_get_stats.argtypes = [vp, C.POINTER(Stats)]
    lib.mihevc_get_headers.argtypes = [vp, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_size_t)]
    lib.mihevc_set_keep_recon.argtypes = [vp, i32]
    lib.mihevc_get_recon.argtypes = [vp, i64, vp, vp, vp]
    lib.mihevc_coded_size.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    lib.mihevc_get_frame_info.argtypes = [vp, i64, C.POINTER(i32), C.POINTER(i32), C.POINTER(i64)]
    lib.mihevc_cost_params_for_qp.argtypes = [i32, i32, i32, C.POINTER(CostParams)]
    lib.mihevc_cost_params_for_qp.restype = None
    lib.mihevc_k_transform.argtypes = [i32, vp, vp, vp, i32, i32, i32, i32, i32, i32]
    lib.mihevc_k_transform_sdh.argtypes = [i32, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32]
    lib.mihevc_k_intra_frame.argtypes = [i32, vp, vp, vp, i32, i32, C.POINTER(CostParams), vp, vp, vp, vp, vp, vp, vp, vp]
    lib.mihevc_k_intra_plan.argtypes = [i32, vp, vp, vp, i32, i32, C.POINTER(CostParams), vp]
    lib.mihevc_k_inter_frame.argtypes = [i32, vp, vp, vp, vp, vp, vp, i32, i32, C.POINTER(CostParams), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.mihevc_k_b_frame.argtypes = [i32] + [vp] * 9 + [i32, i32, C.POINTER(CostParams)] + [vp] * 12
    lib.mihevc_k_deblock.argtypes = [i32, vp, vp, vp, i32, i32, vp, i32]
    lib.mihevc_k_sao.argtypes = [i32, vp, vp, vp, vp, vp, vp, i32, i32, C.POINTER(CostParams), vp, vp, vp, vp]
    lib.mihevc_k_loop_filter.argtypes = [i32, vp, vp, vp, vp, vp, vp, i32, i32, vp, C.POINTER(CostParams), vp, vp, vp, vp]
    lib.mihevc_write_parameter_sets.argtypes = [C.POINTER(Config), vp, C.c_size_t]
    lib.mihevc_encode_picture_host.argtypes = [C.POINTER(Config), i32, i32, i32, vp, vp, vp, vp, vp, vp, C.c_size_t]
    lib.mihevc_k_picture_hash.argtypes = [i32, vp, vp, vp, i32, i32, i32, i32, vp]
    lib.mihevc_write_picture_hash_sei.argtypes = [C.POINTER(Config), i32, vp, vp, C.c_size_t]
    lib.mihevc_get_frame_quality.argtypes = [vp, i64, vp, vp, vp]
    lib.mihevc_k_ssim.argtypes = [i32, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp]
    lib.mihevc_send_frame_fmt.argtypes = [vp, C.POINTER(SrcFormat), vp, vp, vp, i32, i32, i64, i32]
    lib.mihevc_k_convert_source.argtypes = [i32, C.POINTER(SrcFormat), vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp]
    lib.mihevc_send_frame_rgb.argtypes = [vp, C.POINTER(RgbFormat), vp, vp, vp, i32, i64, i32]
    lib.mihevc_k_convert_rgb.argtypes = [i32, C.POINTER(RgbFormat), vp, vp, vp, i32, i32, i32, i32, vp, vp, vp]
    lib.mihevc_send_frame_scaled.argtypes = [vp, C.POINTER(ScaleSrc), vp, vp, vp, i32, i32, i64, i32]
    lib.mihevc_k_scale_source.argtypes = [i32, C.POINTER(ScaleSrc), vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp]
    lib.mihevc_k_scene_diff.argtypes = [i32, vp, vp, i32, i32, i32, i32, vp]
    lib.mihevc_send_frame_deint.argtypes = [vp, C.POINTER(Deint), vp, vp, vp, i32, i32, i64, i32]
    lib.mihevc_k_deinterlace.argtypes = [i32, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), i32, i32, i32, i32, i32, i32, i32, vp, vp, vp]
    lib.mihevc_send_frame_denoise.argtypes = [vp, C.POINTER(Denoise), vp, vp, vp, i32, i32, i64, i32]
    lib.mihevc_k_denoise.argtypes = [i32, C.POINTER(Denoise), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), i32, i32, i32, i32, i32, vp, vp, vp]
    lib.mihevc_send_frame_fieldmatch.argtypes = [vp, C.POINTER(Fieldmatch), vp, vp, vp, i32, i32, i64, i32]
    lib.mihevc_get_fieldmatch_info.argtypes = [vp, i64, C.POINTER(FmFrame)]
    lib.mihevc_k_fieldmatch_metrics.argtypes = [i32, vp, vp, vp, i32, i32, i32, i32, i32, vp]
    lib.mihevc_k_fieldmatch_weave.argtypes = [i32, C.POINTER(vp), C.POINTER(vp), i32, i32, i32, i32, i32, i32, vp, vp, vp]
    lib.mihevc_set_lut3d.argtypes = [vp, i32, vp]
    lib.mihevc_send_frame_lut3d.argtypes = [vp, C.POINTER(Lut3dSrc), vp, vp, vp, i32, i32, i64, i32]
    lib.mihevc_k_lut3d.argtypes = [i32, C.POINTER(Lut3dSrc), i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, C.POINTER(vp), C.POINTER(i32)]
    lib.mihevc_send_frame_interpolate.argtypes = [vp, C.POINTER(Interpolate), vp, vp, vp, i32, i32, i64, i32]
    lib.mihevc_k_mcfi_vectors.argtypes = [i32, vp, vp, i32, i32, i32, i32, vp, vp, vp]
    lib.mihevc_k_mcfi_render.argtypes = [i32, C.POINTER(Interpolate), i32, C.POINTER(vp), C.POINTER(vp), vp, C.c_uint64, i32, i32, i32, i32, i32, vp, vp, vp]
    lib.mihevc_send_frame_upscaled.argtypes = [vp, C.POINTER(UpscaleSrc), vp, vp, vp, i32, i32, i64, i32]
    lib.mihevc_k_upscale_source.argtypes = [i32, C.POINTER(UpscaleSrc), vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp]
    lib.mihevc_set_sr_model.argtypes = [vp, C.POINTER(SrModel), vp, C.c_size_t]
    lib.mihevc_send_frame_sr.argtypes = [vp, C.POINTER(RgbFormat), i32, i32, vp, vp, vp, i32, i64, i32]
    lib.mihevc_k_sr_conv.argtypes = [i32, C.POINTER(SrConvDesc), vp, vp, vp, vp, vp, vp]
    lib.mihevc_k_sr_input.argtypes = [i32, C.POINTER(RgbFormat), i32, i32, i32, vp, vp, vp, i32, vp]
    lib.mihevc_k_sr_network.argtypes = [i32, C.POINTER(SrModel), vp, C.c_size_t, C.POINTER(RgbFormat), i32, i32, vp, vp, vp, i32, vp]
    lib.mihevc_send_frame_sr_yuv.argtypes = [vp, C.POINTER(SrYuv), vp, vp, vp, i32, i32, i64, i32]
    lib.mihevc_send_frame_sr_fit.argtypes = [vp, C.POINTER(RgbFormat), i32, i32, vp, vp, vp, i32, i64, i32]
    lib.mihevc_k_sr_from_yuv.argtypes = [i32, C.POINTER(SrYuv), i32, vp, vp, vp, i32, i32, vp]
    lib.mihevc_set_sr_compact.argtypes = [vp, C.POINTER(SrCompact), vp, C.c_size_t]
    lib.mihevc_k_sr_compact_conv.argtypes = [i32, C.POINTER(SrCompactConvDesc), vp, vp, vp, vp, vp, vp]
    lib.mihevc_k_sr_compact_network.argtypes = [i32, C.POINTER(SrCompact), vp, C.c_size_t, C.POINTER(RgbFormat), i32, i32, vp, vp, vp, i32, vp]
    lib.mihevc_set_source_chain.argtypes = [vp, C.POINTER(Chain)]
    lib.mihevc_send_frame_chain.argtypes = [vp, vp, vp, vp, i32, i32, i64, i32]
    lib.mihevc_chain_plan_for.argtypes = [C.POINTER(Chain), i32, i32, i32, i32, i32, i64, C.POINTER(ChainPlan)]
    _lib = lib
    return lib


def strerror(code: int) -> str:
    try:
        return load().mihevc_strerror(code).decode()
    except Exception:
        return f"mihevc error {code}"


def default_config() -> Config:
    cfg = Config()
    load().mihevc_config_default(C.byref(cfg))
    return cfg


def cost_params(qp: int, bit_depth: int = 8, me_range: int = 16) -> CostParams:
    p = CostParams()
    load().mihevc_cost_params_for_qp(qp, bit_depth, me_range, C.byref(p))
    return p


def p_tile_grid(cfg: Config):
    """(columns, rows) of the tile grid P pictures of this configuration are coded with (mihevc_p_tile_grid); (1, 1) when off."""
    c, r = C.c_int(), C.c_int()
    rc = load().mihevc_p_tile_grid(C.byref(cfg), C.byref(c), C.byref(r))
    if rc != 0:
        raise MihevcError(rc, "mihevc_p_tile_grid")
    return c.value, r.value


def tile_grid(cfg: Config):
    """(columns, rows) of the tile grid IDR pictures of this configuration are coded with (mihevc_tile_grid)."""
    c, r = C.c_int(), C.c_int()
    rc = load().mihevc_tile_grid(C.byref(cfg), C.byref(c), C.byref(r))
    if rc != 0:
        raise MihevcError(rc, "mihevc_tile_grid")
    return c.value, r.value
