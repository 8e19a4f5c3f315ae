"""Python driver of the native MI355X encoder (C ABI in include/mihevc.h, loaded by hevc_amd._lib).

`Encoder` is a thin object wrapper over one `mihevc_session`; `encode_file` is what `convert_video` calls for the
'MI355X' backend: probe -> operating point (the same numbers the reference hands to libx265,
core/transcoder.py:357-412) -> read frames -> session -> Annex-B packets -> MP4 (hvc1).  ctypes releases the GIL
during every call, so N worker threads can each drive their own session like the reference's N QThreads each
block on their own ffmpeg child (gui/worker.py:30-52).
"""
from __future__ import annotations

import ctypes as C
import logging
import re
import threading
from fractions import Fraction
from pathlib import Path
from typing import Callable, Iterator, Optional, Tuple

import numpy as np

from . import _lib
from .probe import VideoInfo

logger = logging.getLogger(__name__)

_COLOUR_CODES = {  # ffprobe names -> H.265 Table E.3/E.4/E.5 code points
    "primaries": {"bt709": 1, "bt470bg": 5, "smpte170m": 6, "bt2020": 9},
    "transfer": {"bt709": 1, "smpte170m": 6, "smpte2084": 16, "pq": 16, "arib-std-b67": 18, "bt2020-10": 14},
    "matrix": {"bt709": 1, "bt470bg": 5, "smpte170m": 6, "bt2020nc": 9, "bt2020-ncl": 9, "bt2020": 9},
}


_DEPTH_IN_FMT = re.compile(r'(?:p|gray|gbrp|yuva?\d{3}p?)(9|10|12|14|16)(?:le|be)?$|^(?:p0|p2|p4|y2)(10|12|16)(?:le|be)?$')


def bit_depth_of(info: VideoInfo) -> int:
    """10 for sample formats deeper than 8 bit (yuv420p10le, p010le, yuv420p12le ... — this path codes Main or Main10, so 12 / 16-bit sources come
    in as 10) and for anything probed as HDR, else 8.  The depth is parsed from the END of the format name: yuv410p / yuvj411p are 8-bit formats
    whose chroma layout happens to spell a '10' or '11'.  Deviation from the reference, documented in INTEGRATION.md §4: its libx265 branch codes
    every non-HDR input as 8-bit Main (core/transcoder.py:363-364); the native path keeps a 10-bit SDR source's samples (Main10, no HDR10 SEI)."""
    if info.hdr:
        return 10
    m = _DEPTH_IN_FMT.search((info.pix_fmt or '').lower())
    return 10 if m and int(m.group(1) or m.group(2)) > 8 else 8


def lanes_for(total_frames: int, keyint: int) -> int:
    """GOP lanes of the session's lock-step pipeline (`gops_in_flight`): a chunk is lanes x keyint pictures and its GOPs run side by side, so a clip
    of up to 8 GOPs is one chunk with every GOP its own lane, longer clips run 8 at a time (a step's fixed part — small kernels, launch ramps, the IDR chain —
    is shared by more pictures: 4609 -> 5150 fps from 4 to 8 lanes on a 1440-frame 1080p clip, no more at 12 or 16); 4 is the floor and what an unknown length gets."""
    if total_frames <= 0 or keyint <= 0:
        return 4
    return max(4, min(8, -(-total_frames // keyint)))


def config_for(info: VideoInfo, crf: int, vbv_maxrate: int, vbv_bufsize: int, gop: int, level: str, tier: str,
               master_display: str = "", max_cll: str = "", sign_hide: int = 0, pic_hash: int = 0, ssim: int = 0) -> _lib.Config:
    """Map the reference's libx265 operating point (build_ffmpeg_params CPU branch) onto a mihevc_config.  sign_hide=1: sign data
    hiding (x265 signhide, on in its presets; off here by default until the measured gain decides).  pic_hash: decoded picture hash
    SEI in every access unit, x265 hash= numbering (0 off, 1 MD5, 2 CRC, 3 checksum).  ssim=1: per-picture SSIM on the device (x265 ssim),
    read with Encoder.frame_quality() and stats().ssim_*; no bit of the stream depends on it."""
    from .utils import parse_master_display, parse_max_cll
    cfg = _lib.default_config()
    cfg.width, cfg.height = int(info.width), int(info.height)
    fr = Fraction(str(info.fps or 30.0)).limit_denominator(1001)
    cfg.fps_num, cfg.fps_den = fr.numerator, fr.denominator
    hdr = bool(info.hdr)
    # bit depth follows the SAMPLE format, not the HDR vote: a 10-bit SDR source is coded Main10 without the HDR10 SEI set
    cfg.bit_depth = bit_depth_of(info)
    cfg.level_idc = int(round(float(level) * 30))
    cfg.tier = 1 if tier == "high" else 0
    cfg.crf, cfg.qp = int(crf), -1
    cfg.vbv_maxrate_kbps, cfg.vbv_bufsize_kbits = int(vbv_maxrate), int(vbv_bufsize)
    cfg.keyint, cfg.min_keyint = int(gop), max(2, int(gop) // 2)
    cfg.gops_in_flight = lanes_for(int(getattr(info, 'nb_frames', 0) or 0), int(gop))
    cfg.sign_hide = int(sign_hide)
    cfg.pic_hash = int(pic_hash)
    cfg.ssim = int(ssim)
    if hdr:   # the HDR10 set of core/utils.py:58-69
        cfg.colour_primaries, cfg.transfer, cfg.matrix = 9, 16, 9
        cfg.chroma_loc, cfg.aud, cfg.repeat_headers, cfg.hdr10, cfg.hrd = 0, 1, 1, 1, 1       # ... hrd=1:aud=1:chromaloc=0:repeat-headers=1
        md = parse_master_display(master_display or info.master_display)
        for i, (x, y) in enumerate((md.g, md.b, md.r)):
            cfg.md_primaries[i][0], cfg.md_primaries[i][1] = x, y
        cfg.md_white[0], cfg.md_white[1] = md.wp
        cfg.md_max_lum, cfg.md_min_lum = md.lum
        cfg.max_cll, cfg.max_fall = parse_max_cll(max_cll or info.max_cll)
    else:
        cfg.colour_primaries = _COLOUR_CODES["primaries"].get(info.color_primaries, 1)
        cfg.transfer = _COLOUR_CODES["transfer"].get(info.color_transfer, 1)
        cfg.matrix = _COLOUR_CODES["matrix"].get(info.color_space, 1)
    return cfg


class Encoder:
    """One encode session on one MI355X.  Raises _lib.MihevcError on any native failure (never falls back)."""

    def __init__(self, cfg: _lib.Config, device: int = 0, keep_recon: bool = False):
        self._lib = _lib.load()
        self.cfg = cfg
        self._s = C.c_void_p()
        rc = self._lib.mihevc_open(C.byref(cfg), device, C.byref(self._s))
        if rc != 0:
            raise _lib.MihevcError(rc, "mihevc_open")
        if keep_recon:
            self._lib.mihevc_set_keep_recon(self._s, 1)
        self._pts = 0
        self._arrays = None     # mihevc_receive_packets' output arrays, made at the first drain and kept
        self._ready = []        # packets received and not yet handed on, last first

    # -- lifecycle
    def close(self):
        if self._s:
            self._lib.mihevc_close(self._s)
            self._s = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc, what):
        if rc != 0:
            detail = self._lib.mihevc_last_error(self._s).decode() if self._s else ""
            raise _lib.MihevcError(rc, f"{what} {detail}".strip())

    # -- data path
    def send(self, y: np.ndarray, u: np.ndarray, v: np.ndarray, pts: Optional[int] = None):
        """Planes as uint8 (8 bit) or uint16 (10 bit) arrays of the DISPLAY size.  Shape and sample width are checked here: the C ABI takes
        plain pointers, so a short plane would be read past its end and 10-bit samples handed to an 8-bit session would wrap modulo 256."""
        c = self.cfg
        dt = np.uint8 if c.bit_depth == 8 else np.uint16
        if y.shape != (c.height, c.width) or u.shape != (c.height // 2, c.width // 2) or v.shape != u.shape:
            raise ValueError(f"plane shapes {y.shape}/{u.shape}/{v.shape} do not match the session's {c.width}x{c.height} 4:2:0")
        for p in (y, u, v):            # a wider container is fine as long as the VALUES fit (tests keep 8-bit pictures in uint16 arrays)
            if p.dtype.itemsize > np.dtype(dt).itemsize and p.size and int(p.max()) >> c.bit_depth:
                raise ValueError(f"{p.dtype} samples up to {int(p.max())} handed to a {c.bit_depth}-bit session (open it with bit_depth 10 or down-convert first)")
        y, u, v = (np.ascontiguousarray(p, dtype=dt) for p in (y, u, v))
        pts = self._pts if pts is None else pts
        self._pts = pts + 1
        self._check(self._lib.mihevc_send_frame(self._s, y.ctypes.data, u.ctypes.data, v.ctypes.data, y.shape[1], u.shape[1], pts), "send_frame")

    def send_async(self, y: np.ndarray, u: np.ndarray, v: np.ndarray, pts: Optional[int] = None):
        """mihevc_send_frame_async: returns with the upload in flight.  The arrays must already have the session's sample type and be C-contiguous (no
        copy is made here, that is the point) and must stay alive and unmodified until sync_uploads() or flush(); page-locked memory makes the copies DMA."""
        c = self.cfg
        dt = np.uint8 if c.bit_depth == 8 else np.uint16
        for p in (y, u, v):
            if p.dtype != dt or not p.flags.c_contiguous:
                raise ValueError("send_async needs C-contiguous planes of the session's sample type")
        if y.shape != (c.height, c.width) or u.shape != (c.height // 2, c.width // 2) or v.shape != u.shape:
            raise ValueError(f"plane shapes {y.shape}/{u.shape}/{v.shape} do not match the session's {c.width}x{c.height} 4:2:0")
        pts = self._pts if pts is None else pts
        self._pts = pts + 1
        self._check(self._lib.mihevc_send_frame_async(self._s, y.ctypes.data, u.ctypes.data, v.ctypes.data, y.shape[1], u.shape[1], pts), "send_frame_async")

    @staticmethod
    def _source_planes(fmt, planes, dt, es, floats, asynchronous, who):
        """The planes of a source in the format `fmt` -> (pointers, pitches in elements, flags).  numpy planes: of the dtype `dt` and C-contiguous when `asynchronous` (no
        copy is made), else of its element size `es` and made so here; otherwise torch tensors on the device, read where they are.  floats: whether the samples
        are floats, which the planes must match; None: only the element size counts.  who: the caller, for the messages."""
        flags = _lib.SRC_ASYNC if asynchronous else 0
        if all(isinstance(p, np.ndarray) for p in planes):
            if asynchronous:
                if any(p.dtype != dt or not p.flags.c_contiguous for p in planes):
                    raise ValueError(f"an asynchronous {who} needs C-contiguous planes of the format's element type")
            elif any(p.dtype.itemsize != es or (floats is not None and (p.dtype.kind == "f") != floats) for p in planes):
                raise ValueError(f"{[str(p.dtype) for p in planes]} planes handed over as {fmt!r}")
            else:
                planes = [np.ascontiguousarray(p, dtype=dt) for p in planes]      # (same size and kind: the bits stay)
            return [p.ctypes.data for p in planes], [p.shape[1] for p in planes], flags
        if any(isinstance(p, np.ndarray) or not p.is_cuda or p.element_size() != es or (floats is not None and p.is_floating_point() != floats) or p.stride(1) != 1
               for p in planes):
            raise ValueError(f"device planes must be tensors on the GPU of the format's element {'size' if floats is None else 'type'} with unit column stride")
        return [p.data_ptr() for p in planes], [p.stride(0) for p in planes], flags | _lib.SRC_DEVICE

    def send_fmt(self, fmt: _lib.SrcFormat, y, u, v, pts: Optional[int] = None, asynchronous: bool = False):
        """mihevc_send_frame_fmt: a picture of the session's display size in another sample layout (4:2:2 / 4:4:4, semi-planar, 8 .. 16 bit), converted on
        the device.  numpy planes (uint8 at 8 bit, else uint16; a semi-planar source: `u` is the interleaved (rows, 2 x chroma width) plane and `v` is None)
        are checked for shape and type here; torch tensors on the session's device are read where they are (MIHEVC_SRC_DEVICE): their producer must have
        finished, and they must stay alive and unmodified until sync_uploads() or flush().  asynchronous (host planes): return with the upload in flight, under
        the rules of send_async."""
        c = self.cfg
        rows, row = fmt.chroma_shape(c.width, c.height)
        planes = [y, u] if fmt.semi_planar else [y, u, v]
        shapes = [(c.height, c.width)] + [(rows, row)] * (len(planes) - 1)
        if any(p is None or tuple(p.shape) != s for p, s in zip(planes, shapes)):
            raise ValueError(f"plane shapes {[None if p is None else tuple(p.shape) for p in planes]} do not match {shapes} of {fmt!r} at {c.width}x{c.height}")
        es = 1 if fmt.bit_depth == 8 else 2
        ptrs, pitches, flags = self._source_planes(fmt, planes, np.dtype(np.uint8 if es == 1 else np.uint16), es, None, asynchronous, "send_fmt")
        if len(planes) == 3 and pitches[1] != pitches[2]:
            raise ValueError("the two chroma planes must share one pitch")
        pts = self._pts if pts is None else pts
        self._pts = pts + 1
        self._check(self._lib.mihevc_send_frame_fmt(self._s, C.byref(fmt), ptrs[0], ptrs[1], ptrs[2] if len(ptrs) == 3 else None, pitches[0], pitches[1], pts, flags),
                    "send_frame_fmt")

    def send_scaled(self, width: int, height: int, y, u, v, bit_depth: Optional[int] = None, pts: Optional[int] = None, asynchronous: bool = False):
        """mihevc_send_frame_scaled: a planar 4:2:0 picture of width x height samples (per axis between the session's size and four times it), scaled down
        to the session's size on the device.  bit_depth: significant bits of a source sample, 8 .. 16 (None: the session's).  numpy planes (uint8 at 8 bit,
        else uint16) are checked for shape and type here; torch tensors on the device are read where they are (MIHEVC_SRC_DEVICE) under the rules of
        send_fmt, and several sessions may be fed from the same tensors.  asynchronous (host planes): the rules of send_async."""
        src = _lib.ScaleSrc(int(width), int(height), int(self.cfg.bit_depth if bit_depth is None else bit_depth))
        planes = [y, u, v]
        shapes = [(src.height, src.width)] + [(src.height // 2, src.width // 2)] * 2
        if any(p is None or tuple(p.shape) != s for p, s in zip(planes, shapes)):
            raise ValueError(f"plane shapes {[None if p is None else tuple(p.shape) for p in planes]} do not match {shapes} of {src!r}")
        es = 1 if src.bit_depth == 8 else 2
        ptrs, pitches, flags = self._source_planes(src, planes, np.dtype(np.uint8 if es == 1 else np.uint16), es, None, asynchronous, "send_scaled")
        if pitches[1] != pitches[2]:
            raise ValueError("the two chroma planes must share one pitch")
        pts = self._pts if pts is None else pts
        self._pts = pts + 1
        self._check(self._lib.mihevc_send_frame_scaled(self._s, C.byref(src), ptrs[0], ptrs[1], ptrs[2], pitches[0], pitches[1], pts, flags), "send_frame_scaled")

    def send_deint(self, y, u, v, tff: bool = True, field_rate: bool = False, asynchronous: bool = False, pts: Optional[int] = None):
        """mihevc_send_frame_deint: a woven interlaced frame of the session's display size, planar 4:2:0 at the session's depth, deinterlaced on the device
        (DESIGN.md §6f).  tff: the top field (even rows) is the first in time.  field_rate: two pictures per frame, pts and pts + 1: the session is opened at
        twice the frame rate and pts counts field periods (the default pts advances by 2).  The frame's picture(s) come out once the next frame has arrived,
        the last frame's with flush().  Width even, height a multiple of 4, both at least 16; field order and rate are those of the first call.  numpy planes
        are checked for shape and type here; torch tensors on the device are read where they are (MIHEVC_SRC_DEVICE) under the rules of send_fmt.
        asynchronous (host planes): the rules of send_async."""
        c = self.cfg
        mode = _lib.Deint(int(bool(tff)), int(bool(field_rate)))
        planes = [y, u, v]
        shapes = [(c.height, c.width)] + [(c.height // 2, c.width // 2)] * 2
        if any(p is None or tuple(p.shape) != s for p, s in zip(planes, shapes)):
            raise ValueError(f"plane shapes {[None if p is None else tuple(p.shape) for p in planes]} do not match {shapes} of the session")
        es = 1 if c.bit_depth == 8 else 2
        ptrs, pitches, flags = self._source_planes(mode, planes, np.dtype(np.uint8 if es == 1 else np.uint16), es, None, asynchronous, "send_deint")
        if pitches[1] != pitches[2]:
            raise ValueError("the two chroma planes must share one pitch")
        pts = self._pts if pts is None else pts
        self._pts = pts + (2 if field_rate else 1)
        self._check(self._lib.mihevc_send_frame_deint(self._s, C.byref(mode), ptrs[0], ptrs[1], ptrs[2], pitches[0], pitches[1], pts, flags), "send_frame_deint")

    def send_fieldmatch(self, y, u, v, tff: bool = True, decimate: bool = True, deint: bool = True, asynchronous: bool = False, pts: Optional[int] = None):
        """mihevc_send_frame_fieldmatch: a woven frame of the session's display size, planar 4:2:0 at the session's depth, that carries film in fields (3:2
        pulldown): inverse telecine on the device.  tff: the declared field order.  decimate: of every five frames the repeat is dropped and the
        pictures are numbered pts_first, pts_first + 1, ...: the session is opened at 4/5 of the source rate.  deint: frames that stay combed are deinterlaced.
        A frame is decided once the next one has arrived, the last one with flush(); with decimate its picture waits for the cycle's fifth frame.  Every call
        waits for the metrics of the frame before, so an asynchronous one returns with less in flight than send_async does.  Geometry, planes and the mode of
        the first call: the rules of send_deint; no other send_* may follow before flush()."""
        c = self.cfg
        mode = _lib.Fieldmatch(int(bool(tff)), int(bool(decimate)), int(bool(deint)))
        planes = [y, u, v]
        shapes = [(c.height, c.width)] + [(c.height // 2, c.width // 2)] * 2
        if any(p is None or tuple(p.shape) != s for p, s in zip(planes, shapes)):
            raise ValueError(f"plane shapes {[None if p is None else tuple(p.shape) for p in planes]} do not match {shapes} of the session")
        es = 1 if c.bit_depth == 8 else 2
        ptrs, pitches, flags = self._source_planes(mode, planes, np.dtype(np.uint8 if es == 1 else np.uint16), es, None, asynchronous, "send_fieldmatch")
        if pitches[1] != pitches[2]:
            raise ValueError("the two chroma planes must share one pitch")
        pts = self._pts if pts is None else pts
        self._pts = pts + 1
        self._check(self._lib.mihevc_send_frame_fieldmatch(self._s, C.byref(mode), ptrs[0], ptrs[1], ptrs[2], pitches[0], pitches[1], pts, flags), "send_frame_fieldmatch")

    def fieldmatch_info(self, i: int):
        """mihevc_get_fieldmatch_info: the _lib.FmFrame of fieldmatch frame i (metrics, match, deinterlaced, dropped, picture), or None while it is undecided"""
        out = _lib.FmFrame()
        rc = self._lib.mihevc_get_fieldmatch_info(self._s, int(i), C.byref(out))
        if rc == _lib.EAGAIN:
            return None
        self._check(rc, "get_fieldmatch_info")
        return out

    def send_denoise(self, y, u, v, strength=2, asynchronous: bool = False, pts: Optional[int] = None):
        """mihevc_send_frame_denoise: a progressive frame of the session's display size, planar 4:2:0 at the session's depth, denoised on the device by the
        motion-adaptive spatio-temporal filter of DESIGN.md §6g.  strength: a level 0 .. 3 (_lib.denoise_level), a tuple (luma_spatial, luma_temporal,
        chroma_spatial, chroma_temporal) of thresholds 0 .. 255 in 8-bit units, or a _lib.Denoise; it belongs to this frame and may change from frame to frame.
        The frame's picture comes out once the next frame has arrived, the last frame's with flush().  Width and height even and at least 16.  numpy planes are
        checked for shape and type here; torch tensors on the device are read where they are (MIHEVC_SRC_DEVICE) under the rules of send_fmt.  asynchronous
        (host planes): the rules of send_async."""
        c = self.cfg
        dn = strength if isinstance(strength, _lib.Denoise) else _lib.denoise_strength(strength)
        planes = [y, u, v]
        shapes = [(c.height, c.width)] + [(c.height // 2, c.width // 2)] * 2
        if any(p is None or tuple(p.shape) != s for p, s in zip(planes, shapes)):
            raise ValueError(f"plane shapes {[None if p is None else tuple(p.shape) for p in planes]} do not match {shapes} of the session")
        es = 1 if c.bit_depth == 8 else 2
        ptrs, pitches, flags = self._source_planes(dn, planes, np.dtype(np.uint8 if es == 1 else np.uint16), es, None, asynchronous, "send_denoise")
        if pitches[1] != pitches[2]:
            raise ValueError("the two chroma planes must share one pitch")
        pts = self._pts if pts is None else pts
        self._pts = pts + 1
        self._check(self._lib.mihevc_send_frame_denoise(self._s, C.byref(dn), ptrs[0], ptrs[1], ptrs[2], pitches[0], pitches[1], pts, flags), "send_frame_denoise")

    def send_interpolate(self, y, u, v, factor: int = 2, mode: str = 'mc', scene_threshold: int = 10, asynchronous: bool = False, pts: Optional[int] = None):
        """mihevc_send_frame_interpolate: a progressive frame of the session's display size, planar 4:2:0 at the session's depth; between it and the next frame
        factor - 1 pictures are interpolated on the device.  factor: 2, 3 or 4 pictures per frame; mode: 'mc' (motion compensated) or 'blend';
        both are those of the session's first call.  scene_threshold: 0 .. 255 in 8-bit units of mean absolute luma difference, 0 for no scene check; a pair of
        frames above it repeats its nearer frame.  Frame k's pictures come out at pts, pts + 1, .. once the next frame has arrived, the last frame's own picture
        with flush(): the caller numbers pts `factor` apart (the default does) and opens the session at factor times the source rate.  Width and height even and
        at least 16.  Planes and asynchronous: the rules of send_denoise."""
        c = self.cfg
        m = _lib.interpolate_mode(factor, mode, scene_threshold)
        planes = [y, u, v]
        shapes = [(c.height, c.width)] + [(c.height // 2, c.width // 2)] * 2
        if any(p is None or tuple(p.shape) != s for p, s in zip(planes, shapes)):
            raise ValueError(f"plane shapes {[None if p is None else tuple(p.shape) for p in planes]} do not match {shapes} of the session")
        es = 1 if c.bit_depth == 8 else 2
        ptrs, pitches, flags = self._source_planes(m, planes, np.dtype(np.uint8 if es == 1 else np.uint16), es, None, asynchronous, "send_interpolate")
        if pitches[1] != pitches[2]:
            raise ValueError("the two chroma planes must share one pitch")
        pts = self._pts if pts is None else pts
        self._pts = pts + m.factor
        self._check(self._lib.mihevc_send_frame_interpolate(self._s, C.byref(m), ptrs[0], ptrs[1], ptrs[2], pitches[0], pitches[1], pts, flags), "send_frame_interpolate")

    def set_chain(self, width: int, height: int, bit_depth: Optional[int] = None, **stages):
        """mihevc_set_source_chain: the source filters in series, set once before the first frame; every frame then goes through send_chain and no
        other send_*.  width, height, bit_depth (None: the session's): the source.  The stages, in their fixed order, are the keywords of _lib.chain: field=None |
        'deint' (tff, field_rate) | 'fieldmatch' (tff, decimate, fm_deint); denoise=None | a level or four thresholds; resize=None | 'scale' | 'upscale' (sharpen,
        antiring) | 'sr' (sr_matrix, sr_full_range; the model of set_sr_model, set before this call); interpolate=None | 2 .. 4 (interp_mode, scene_threshold).  A
        _lib.Chain as the only stage argument `chain=` is taken as it is.  Returns the _lib.Chain."""
        c = stages.pop("chain") if "chain" in stages else _lib.chain(width, height, self.cfg.bit_depth if bit_depth is None else bit_depth, **stages)
        self._check(self._lib.mihevc_set_source_chain(self._s, C.byref(c)), "set_source_chain")
        self._chain = c
        return c

    def send_chain(self, y, u, v, pts: Optional[int] = None, asynchronous: bool = False):
        """mihevc_send_frame_chain: a planar 4:2:0 frame of the chain's source size and depth through the chain of set_chain.  The pictures are numbered
        consecutively from the first frame's pts: the session is opened at the source's rate times the chain's (_lib.chain_plan).  What comes out when is the
        stages' own: every temporal stage holds its last frame back until the next one arrives, and flush() drains them front to back.  numpy planes are checked
        for shape and type here; torch tensors on the device are read where they are (MIHEVC_SRC_DEVICE) under the rules of send_fmt.  asynchronous (host planes):
        the rules of send_async."""
        c = getattr(self, "_chain", None)
        if c is None:
            raise _lib.MihevcError(_lib.ESTATE, "send_chain without set_chain")
        planes = [y, u, v]
        shapes = [(c.height, c.width)] + [(c.height // 2, c.width // 2)] * 2
        if any(p is None or tuple(p.shape) != s for p, s in zip(planes, shapes)):
            raise ValueError(f"plane shapes {[None if p is None else tuple(p.shape) for p in planes]} do not match {shapes} of {c!r}")
        es = 1 if c.bit_depth == 8 else 2
        ptrs, pitches, flags = self._source_planes(c, planes, np.dtype(np.uint8 if es == 1 else np.uint16), es, None, asynchronous, "send_chain")
        if pitches[1] != pitches[2]:
            raise ValueError("the two chroma planes must share one pitch")
        pts = self._pts if pts is None else pts
        self._pts = pts + 1
        self._check(self._lib.mihevc_send_frame_chain(self._s, ptrs[0], ptrs[1], ptrs[2], pitches[0], pitches[1], pts, flags), "send_frame_chain")

    def set_lut3d(self, table):
        """mihevc_set_lut3d: the 3D colour table send_lut3d interpolates in: an (n, n, n, 3) array indexed [b][g][r][c], the order of a .cube
        file, 2 <= n <= 65; uint16 entries 0 .. 65535, or floats in [0, 1] that go through lut3d.quantise first.  It is copied before the call returns and may be
        replaced between frames: frames already sent keep the table they were sent under.  None drops the table."""
        if table is None:
            self._check(self._lib.mihevc_set_lut3d(self._s, 0, None), "set_lut3d")
            return
        from . import lut3d
        t = lut3d.as_uint16(table)
        self._check(self._lib.mihevc_set_lut3d(self._s, t.shape[0], t.ctypes.data), "set_lut3d")

    def send_lut3d(self, y, u, v, bit_depth: int, matrix: int, full_range: bool = False, pts: Optional[int] = None, asynchronous: bool = False):
        """mihevc_send_frame_lut3d: a planar 4:2:0 Y'CbCr picture of the session's display size at bit_depth 8, 10 or 12 with its own matrix (1, 5, 6 or 9) and
        range, taken through the table of set_lut3d on the device and coded with the session's matrix, range and depth (an HDR master into an SDR stream).
        numpy planes (uint8 at 8 bit, else uint16) are checked for shape and type here; torch tensors on the device are read where they are
        (MIHEVC_SRC_DEVICE) under the rules of send_fmt.  asynchronous (host planes): the rules of send_async."""
        c = self.cfg
        src = _lib.Lut3dSrc(int(bit_depth), int(matrix), 1 if full_range else 0)
        planes = [y, u, v]
        shapes = [(c.height, c.width)] + [(c.height // 2, c.width // 2)] * 2
        if any(p is None or tuple(p.shape) != s for p, s in zip(planes, shapes)):
            raise ValueError(f"plane shapes {[None if p is None else tuple(p.shape) for p in planes]} do not match {shapes} of the session")
        es = 1 if src.bit_depth == 8 else 2
        ptrs, pitches, flags = self._source_planes(src, planes, np.dtype(np.uint8 if es == 1 else np.uint16), es, None, asynchronous, "send_lut3d")
        if pitches[1] != pitches[2]:
            raise ValueError("the two chroma planes must share one pitch")
        pts = self._pts if pts is None else pts
        self._pts = pts + 1
        self._check(self._lib.mihevc_send_frame_lut3d(self._s, C.byref(src), ptrs[0], ptrs[1], ptrs[2], pitches[0], pitches[1], pts, flags), "send_frame_lut3d")

    def send_upscaled(self, width: int, height: int, y, u, v, bit_depth: Optional[int] = None, sharpen: int = 8, antiring: int = 8, pts: Optional[int] = None,
                      asynchronous: bool = False):
        """mihevc_send_frame_upscaled: a planar 4:2:0 picture of width x height samples (per axis between a quarter of the session's size and that size), enlarged
        to the session's size on the device: Catmull-Rom interpolation, blended `antiring` eighths (0 .. 8) into the range of the two nearest
        samples, then on luma a limited 3x3 sharpener of gain `sharpen` sixteenths (0 .. 64, 0: off); both may change from picture to picture.  bit_depth,
        the planes and asynchronous: as send_scaled."""
        src = _lib.UpscaleSrc(int(width), int(height), int(self.cfg.bit_depth if bit_depth is None else bit_depth), int(sharpen), int(antiring))
        planes = [y, u, v]
        shapes = [(src.height, src.width)] + [(src.height // 2, src.width // 2)] * 2
        if any(p is None or tuple(p.shape) != s for p, s in zip(planes, shapes)):
            raise ValueError(f"plane shapes {[None if p is None else tuple(p.shape) for p in planes]} do not match {shapes} of {src!r}")
        es = 1 if src.bit_depth == 8 else 2
        ptrs, pitches, flags = self._source_planes(src, planes, np.dtype(np.uint8 if es == 1 else np.uint16), es, None, asynchronous, "send_upscaled")
        if pitches[1] != pitches[2]:
            raise ValueError("the two chroma planes must share one pitch")
        pts = self._pts if pts is None else pts
        self._pts = pts + 1
        self._check(self._lib.mihevc_send_frame_upscaled(self._s, C.byref(src), ptrs[0], ptrs[1], ptrs[2], pitches[0], pitches[1], pts, flags), "send_frame_upscaled")

    def set_sr_model(self, model):
        """mihevc_set_sr_model / mihevc_set_sr_compact: the network send_sr runs: an hevc_amd.sr.RrdbNet (load_rrdbnet), an hevc_amd.sr.CompactNet
        (load_compact, blend; §6m), or None to drop the model.  A session has one model: setting one of either kind replaces the other.  The weights are packed
        and on their way to the device before the call returns; a model may be replaced between frames, and frames already sent keep theirs."""
        if model is None:
            self._check(self._lib.mihevc_set_sr_model(self._s, None, None, 0), "set_sr_model")
            return
        w = np.ascontiguousarray(model.weights, dtype=np.float32)
        if hasattr(model, "convs"):
            m = _lib.SrCompact(int(model.scale), int(model.convs))
            self._check(self._lib.mihevc_set_sr_compact(self._s, C.byref(m), w.ctypes.data, w.size), "set_sr_compact")
            return
        m = _lib.SrModel(int(model.scale), int(model.blocks))
        self._check(self._lib.mihevc_set_sr_model(self._s, C.byref(m), w.ctypes.data, w.size), "set_sr_model")

    def send_sr(self, fmt: _lib.RgbFormat, width: int, height: int, *planes, pts: Optional[int] = None, asynchronous: bool = False, _entry: str = "send_frame_sr"):
        """mihevc_send_frame_sr: a full-range R'G'B' picture of width x height, enlarged by the model of set_sr_model into the session's size (scale x the
        source's), then converted as send_rgb converts.  The planes, their types, torch tensors on the device and `asynchronous`: as send_rgb, at the SOURCE size."""
        width, height = int(width), int(height)
        shapes = fmt.plane_shapes(width, height)
        planes = list(planes)
        if fmt.layout and len(planes) == 1 and planes[0] is not None and tuple(planes[0].shape) == (height, width, fmt.layout):
            if isinstance(planes[0], np.ndarray) or planes[0].is_contiguous():
                planes[0] = planes[0].reshape(height, width * fmt.layout)
        if len(planes) != len(shapes) or any(p is None or tuple(p.shape) != s for p, s in zip(planes, shapes)):
            raise ValueError(f"plane shapes {[None if p is None else tuple(p.shape) for p in planes]} do not match {shapes} of {fmt!r} at {width}x{height}")
        es = fmt.element_size
        dt = np.dtype({1: np.float16, 2: np.float32}[fmt.sample]) if fmt.sample else np.dtype(np.uint8 if es == 1 else np.uint16)
        ptrs, pitches, flags = self._source_planes(fmt, planes, dt, es, bool(fmt.sample), asynchronous, "send_sr")
        if len(set(pitches)) != 1:
            raise ValueError("the three planes must share one pitch")
        pts = self._pts if pts is None else pts
        self._pts = pts + 1
        ptrs += [None] * (3 - len(ptrs))
        self._check(getattr(self._lib, "mihevc_" + _entry)(self._s, C.byref(fmt), width, height, ptrs[0], ptrs[1], ptrs[2], pitches[0], pts, flags), _entry)

    def send_sr_fit(self, fmt: _lib.RgbFormat, width: int, height: int, *planes, pts: Optional[int] = None, asynchronous: bool = False):
        """mihevc_send_frame_sr_fit: send_sr into a session that is scale x the source or smaller (per axis down to a quarter of the network's output, every
        size even and at least 16: sr_target_size states the rule); a smaller session gets the network's picture scaled down on the device by the filter of
        send_scaled.  Everything else as send_sr."""
        self.send_sr(fmt, width, height, *planes, pts=pts, asynchronous=asynchronous, _entry="send_frame_sr_fit")

    def send_sr_yuv(self, width: int, height: int, y, u, v, bit_depth: int = 8, matrix: int = 6, full_range: bool = False, pts: Optional[int] = None,
                    asynchronous: bool = False):
        """mihevc_send_frame_sr_yuv: a planar 4:2:0 Y'CbCr picture of width x height (both even) at bit_depth 8, 10 or 12 with its own matrix (1, 5, 6 or 9) and
        range, brought to R'G'B' on the device with the exact integer arithmetic of send_lut3d, enlarged by the model of set_sr_model and coded with the session's
        matrix, range and depth.  The session's size follows the rule of send_sr_fit.  numpy planes (uint8 at 8 bit, else uint16) are checked for shape and type
        here; torch tensors on the device are read where they are (MIHEVC_SRC_DEVICE) under the rules of send_fmt.  asynchronous (host planes): the rules of
        send_async."""
        src = _lib.SrYuv(int(width), int(height), int(bit_depth), int(matrix), 1 if full_range else 0)
        planes = [y, u, v]
        shapes = [(src.height, src.width)] + [(src.height // 2, src.width // 2)] * 2
        if any(p is None or tuple(p.shape) != s for p, s in zip(planes, shapes)):
            raise ValueError(f"plane shapes {[None if p is None else tuple(p.shape) for p in planes]} do not match {shapes} of {src!r}")
        es = 1 if src.bit_depth == 8 else 2
        ptrs, pitches, flags = self._source_planes(src, planes, np.dtype(np.uint8 if es == 1 else np.uint16), es, None, asynchronous, "send_sr_yuv")
        if pitches[1] != pitches[2]:
            raise ValueError("the two chroma planes must share one pitch")
        pts = self._pts if pts is None else pts
        self._pts = pts + 1
        self._check(self._lib.mihevc_send_frame_sr_yuv(self._s, C.byref(src), ptrs[0], ptrs[1], ptrs[2], pitches[0], pitches[1], pts, flags), "send_frame_sr_yuv")

    def send_sr_tensor(self, t, pts: Optional[int] = None, asynchronous: bool = False):
        """send_sr for one tensor in R, G, B order, the shapes and types of send_rgb_tensor; its own size is the source size"""
        fmt, planes = self._rgb_tensor_planes(t, "send_sr_tensor")
        h, w = (int(t.shape[1]), int(t.shape[2])) if fmt.layout == 0 else (int(t.shape[0]), int(t.shape[1]))
        self.send_sr(fmt, w, h, *planes, pts=pts, asynchronous=asynchronous)

    def send_rgb(self, fmt: _lib.RgbFormat, *planes, pts: Optional[int] = None, asynchronous: bool = False):
        """mihevc_send_frame_rgb: a full-range R'G'B' picture of the session's display size, matrixed, range-scaled and decimated to 4:2:0 on the device.
        Three (height, width) planes in the order the format's r / g / b fields index, or one packed plane of shape (height, layout * width) or (height, width,
        layout); uint8 at 8 bit, uint16 above, float16 / float32 for the float formats.  numpy planes are checked for shape and type here; torch tensors on the
        session's device are read where they are (MIHEVC_SRC_DEVICE) under the rules of send_fmt, and so is `asynchronous`."""
        c = self.cfg
        shapes = fmt.plane_shapes(c.width, c.height)
        planes = list(planes)
        if fmt.layout and len(planes) == 1 and planes[0] is not None and tuple(planes[0].shape) == (c.height, c.width, fmt.layout):
            if isinstance(planes[0], np.ndarray) or planes[0].is_contiguous():
                planes[0] = planes[0].reshape(c.height, c.width * fmt.layout)
        if len(planes) != len(shapes) or any(p is None or tuple(p.shape) != s for p, s in zip(planes, shapes)):
            raise ValueError(f"plane shapes {[None if p is None else tuple(p.shape) for p in planes]} do not match {shapes} of {fmt!r} at {c.width}x{c.height}")
        es = fmt.element_size
        dt = np.dtype({1: np.float16, 2: np.float32}[fmt.sample]) if fmt.sample else np.dtype(np.uint8 if es == 1 else np.uint16)
        ptrs, pitches, flags = self._source_planes(fmt, planes, dt, es, bool(fmt.sample), asynchronous, "send_rgb")
        if len(set(pitches)) != 1:
            raise ValueError("the three planes must share one pitch")
        pts = self._pts if pts is None else pts
        self._pts = pts + 1
        ptrs += [None] * (3 - len(ptrs))
        self._check(self._lib.mihevc_send_frame_rgb(self._s, C.byref(fmt), ptrs[0], ptrs[1], ptrs[2], pitches[0], pts, flags), "send_frame_rgb")

    @staticmethod
    def _rgb_tensor_planes(t, who):
        """the format and planes of a tensor send_rgb_tensor / send_sr_tensor take"""
        kind = str(getattr(t, "dtype", "")).rsplit(".", 1)[-1]      # the tensor is taken by its interface: the package does not import torch
        if not hasattr(t, "data_ptr") or t.dim() != 3:
            raise ValueError(f"{who} takes a (3, H, W) or (H, W, 3 | 4) torch tensor")
        if t.shape[0] == 3 and kind in ("uint8", "int16", "uint16", "float16", "float32"):
            sample = 1 if kind == "float16" else 2 if kind == "float32" else 0
            fmt = _lib.RgbFormat(0, 0, 1, 2, sample, 0 if sample else 8 if kind == "uint8" else 16)
            if t.stride(2) != 1 or t.stride(1) < t.shape[2]:
                raise ValueError(f"strides {tuple(t.stride())}: the kernel reads rows of adjacent samples")
            planes = [t[0], t[1], t[2]]
        elif t.shape[2] in (3, 4) and kind == "uint8":
            fmt = _lib.RgbFormat(int(t.shape[2]), 0, 1, 2, 0, 8)
            if t.stride(2) != 1 or t.stride(1) != t.shape[2] or t.stride(0) < t.shape[1] * t.shape[2]:
                raise ValueError(f"strides {tuple(t.stride())}: the kernel reads rows of adjacent pixels")
            planes = [t.as_strided((t.shape[0], t.shape[1] * t.shape[2]), (t.stride(0), 1))]
        else:
            raise ValueError(f"a {tuple(t.shape)} {t.dtype} tensor is no RGB picture this entry takes")
        if not t.is_cuda:
            planes = [p.contiguous().numpy() for p in planes]
            planes = [p.view(np.uint16) if p.dtype == np.int16 else p for p in planes]
        return fmt, planes

    def send_rgb_tensor(self, t, pts: Optional[int] = None, asynchronous: bool = False):
        """send_rgb for one tensor in R, G, B order: (3, H, W) of uint8, 16-bit integers (int16 carries the bits of a uint16), float16 or float32 in [0, 1],
        or (H, W, 3) / (H, W, 4) of uint8 (a fourth element is ignored).  The format is built here; matrix and range follow the session.  A tensor on the session's
        device is read where it is; a layout the kernel cannot read (column stride other than 1, pixels not side by side) raises ValueError."""
        fmt, planes = self._rgb_tensor_planes(t, "send_rgb_tensor")
        self.send_rgb(fmt, *planes, pts=pts, asynchronous=asynchronous)

    def sync_uploads(self):
        self._check(self._lib.mihevc_sync_uploads(self._s), "sync_uploads")

    def send_device(self, y_ptr: int, u_ptr: int, v_ptr: int, pitch_y: int, pitch_c: int, pts: Optional[int] = None):
        pts = self._pts if pts is None else pts
        self._pts = pts + 1
        self._check(self._lib.mihevc_send_frame_device(self._s, y_ptr, u_ptr, v_ptr, pitch_y, pitch_c, pts), "send_frame_device")

    def send_device_batch(self, y_ptrs, u_ptrs, v_ptrs, pitch_y: int, pitch_c: int, first_pts: Optional[int] = None):
        """mihevc_send_frames_device: len(y_ptrs) pictures already in device memory in ONE call.  The pointer lists may be ctypes arrays of c_void_p made once
        for frames that stay where they are (device_pointer_arrays)."""
        n = len(y_ptrs)
        arrs = [p if isinstance(p, C.Array) else (C.c_void_p * n)(*p) for p in (y_ptrs, u_ptrs, v_ptrs)]
        pts = self._pts if first_pts is None else first_pts
        self._pts = pts + n
        self._check(self._lib.mihevc_send_frames_device(self._s, n, arrs[0], arrs[1], arrs[2], pitch_y, pitch_c, pts), "send_frames_device")

    def flush(self):
        self._check(self._lib.mihevc_flush(self._s), "flush")

    def abort(self):
        """mihevc_abort: give the session up (every later call fails; sessions of the same picture's other slices stop waiting for it)"""
        if self._s:
            self._lib.mihevc_abort(self._s)

    _BATCH = 512      # packets per mihevc_receive_packets call: a 300-picture clip drains in one

    def _receive_batch(self) -> bool:
        """One mihevc_receive_packets call into the arrays the Encoder keeps: the ready packets, copied out as (bytes, pts, keyframe, dts), wait in self._ready
        (last first) until a generator hands them on, so a caller that stops iterating early finds the rest in its next packets() call.  False: nothing was ready."""
        if self._arrays is None:
            n = self._BATCH
            self._arrays = ((C.c_void_p * n)(), (C.c_size_t * n)(), (C.c_int64 * n)(), (C.c_int64 * n)(), (C.c_int * n)())
        data, size, pts, dts, key = self._arrays
        n = self._lib.mihevc_receive_packets(self._s, self._BATCH, data, size, pts, dts, key)
        if n in (_lib.EAGAIN, _lib.EOF):
            return False
        if n < 0:
            self._check(n, "receive_packets")
        at = C.string_at
        self._ready = [(at(d, s), p, k != 0, t) for d, s, p, k, t in zip(data[:n], size[:n], pts[:n], key[:n], dts[:n])][::-1]
        return True

    def packets(self) -> Iterator[Tuple[bytes, int, bool]]:
        """Drain every packet that is ready: (annexb bytes, pts, keyframe)."""
        while self._ready or self._receive_batch():
            yield self._ready.pop()[:3]

    def packets_dts(self) -> Iterator[Tuple[bytes, int, bool, int]]:
        """The same with the decoding time stamp: (annexb bytes, pts, keyframe, dts).  Packets always come in DECODING order; dts differs from pts only
        when the session codes B pictures (cfg.bframes)."""
        while self._ready or self._receive_batch():
            yield self._ready.pop()

    def headers(self) -> bytes:
        data, size = C.POINTER(C.c_uint8)(), C.c_size_t()
        self._check(self._lib.mihevc_get_headers(self._s, C.byref(data), C.byref(size)), "get_headers")
        return C.string_at(data, size.value)

    def stats(self) -> _lib.Stats:
        st = _lib.Stats()
        self._check(self._lib.mihevc_get_stats(self._s, C.byref(st)), "get_stats")
        return st

    def coded_size(self) -> Tuple[int, int]:
        w, h = C.c_int(), C.c_int()
        self._lib.mihevc_coded_size(self._s, C.byref(w), C.byref(h))
        return w.value, h.value

    def recon(self, index: int):
        w, h = self.coded_size()
        y, u, v = np.zeros((h, w), np.uint16), np.zeros((h // 2, w // 2), np.uint16), np.zeros((h // 2, w // 2), np.uint16)
        self._check(self._lib.mihevc_get_recon(self._s, index, y.ctypes.data, u.ctypes.data, v.ctypes.data), "get_recon")
        return y, u, v

    def frame_info(self, index: int):
        """(qp, slice_type, bits) of output picture `index`"""
        qp, st, bits = C.c_int(), C.c_int(), C.c_int64()
        self._check(self._lib.mihevc_get_frame_info(self._s, index, C.byref(qp), C.byref(st), C.byref(bits)), "get_frame_info")
        return qp.value, st.value, bits.value

    def frame_quality(self, index: int) -> dict:
        """Quality of output picture `index` (display order) over the coded size, per plane (Y, Cb, Cr): {"sse": squared error of the final reconstruction
        against the source, "psnr": dB (99.0 at zero error), "ssim": mean SSIM of the picture's 8x8 windows, or None when the session runs without cfg.ssim,
        "ssim_q32" / "ssim_windows": the exact integers behind it (None likewise)}"""
        sse, q32, win = (C.c_uint64 * 3)(), (C.c_int64 * 3)(), (C.c_int64 * 3)()
        on = bool(self.cfg.ssim)
        self._check(self._lib.mihevc_get_frame_quality(self._s, index, sse, q32 if on else None, win if on else None), "get_frame_quality")
        w, h = self.coded_size()
        peak = float((1 << self.cfg.bit_depth) - 1)
        n = (w * h, w * h // 4, w * h // 4)
        return {"sse": [int(x) for x in sse],
                "psnr": [99.0 if s == 0 else float(10 * np.log10(peak * peak * k / s)) for s, k in zip(sse, n)],
                "ssim": [q / (k * 4294967296.0) for q, k in zip(q32, win)] if on else None,
                "ssim_q32": [int(x) for x in q32] if on else None, "ssim_windows": [int(x) for x in win] if on else None}

    def psnr_y(self) -> float:
        st = self.stats()
        n = max(1, st.frames_out) * self.coded_size()[0] * self.coded_size()[1]
        peak = (1 << self.cfg.bit_depth) - 1
        mse = st.sse_y / n
        return 99.0 if mse <= 0 else float(10 * np.log10(peak * peak / mse))


class ShardedEncoder:
    """One clip over several MI355X: closed GOPs are independent, so consecutive chunks of `gops_in_flight x keyint` pictures go
    round-robin to one session per device (SURVEY.md §8e "GOP g -> device g mod n"); nothing is exchanged between the devices
    (no RCCL) and the packets come back in presentation order.  `devices` may name a device twice (two sessions on one GPU)."""

    def __init__(self, cfg: _lib.Config, devices):
        import queue
        self.cfg, self.devices = cfg, list(devices)
        lanes = cfg.gops_in_flight if cfg.gops_in_flight > 0 else 4
        self.chunk = max(1, lanes * cfg.keyint)
        self._encs = [Encoder(cfg, device=d) for d in self.devices]
        self._q = [queue.Queue(maxsize=2 * self.chunk) for _ in self.devices]
        self._out = {}                      # pts -> (data, key)
        self._lock = threading.Lock()
        self._err = []
        self._threads = [threading.Thread(target=self._worker, args=(k,), daemon=True) for k in range(len(self.devices))]
        for t in self._threads:
            t.start()
        self._n_in, self._next_out = 0, 0
        self._aborted = False

    def _worker(self, k):
        enc, q = self._encs[k], self._q[k]
        try:
            while True:
                item = q.get()
                if item is None:
                    break
                y, u, v, pts, fmt = item
                if fmt is None:
                    enc.send(y, u, v, pts=pts)      # ctypes releases the GIL: the sessions run concurrently
                elif isinstance(fmt, _lib.RgbFormat):
                    enc.send_rgb(fmt, *[p for p in (y, u, v) if p is not None], pts=pts)
                else:
                    enc.send_fmt(fmt, y, u, v, pts=pts)
                self._collect(enc)
            if not self._aborted:
                enc.flush()
                self._collect(enc)
        except Exception as exc:                    # surfaced by send()/finish() on the caller's thread
            self._err.append(exc)

    def _collect(self, enc):
        got = list(enc.packets())
        if got:
            with self._lock:
                for data, pts, key in got:
                    self._out[pts] = (data, key)

    def send(self, y, u, v, fmt=None):
        """fmt: the planes' _lib.SrcFormat when they are not the session's own layout (Encoder.send_fmt), or their _lib.RgbFormat (Encoder.send_rgb; a packed
        source: y is the packed plane, u and v are None)"""
        import queue
        k = (self._n_in // self.chunk) % len(self.devices)
        while True:                                 # a bounded queue whose worker has died must not block the caller for ever
            if self._err:
                raise self._err[0]
            try:
                self._q[k].put((y, u, v, self._n_in, fmt), timeout=0.2)
                break
            except queue.Full:
                continue
        self._n_in += 1

    def ready(self):
        """Packets that are next in presentation order: (data, pts, key)."""
        out = []
        with self._lock:
            while self._next_out in self._out:
                data, key = self._out.pop(self._next_out)
                out.append((data, self._next_out, key))
                self._next_out += 1
        return out

    def _stop_workers(self, drain: bool):
        """Hand every worker its sentinel and join it; drain=True first throws away what is still queued (abort)."""
        import queue
        for q, t in zip(self._q, self._threads):
            while t.is_alive():
                if drain:
                    try:
                        while True:
                            q.get_nowait()
                    except queue.Empty:
                        pass
                try:
                    q.put(None, timeout=0.2)
                    break
                except queue.Full:
                    continue
        for t in self._threads:
            t.join()

    def finish(self):
        self._stop_workers(drain=False)
        if self._err:
            raise self._err[0]
        return self.ready()

    def abort(self):
        """Cancel / failure path: no session may be closed while its worker can still be inside a native call."""
        self._aborted = True
        self._stop_workers(drain=True)

    def headers(self) -> bytes:
        return self._encs[0].headers()

    def stats(self):
        return [e.stats() for e in self._encs]

    def close(self):
        if any(t.is_alive() for t in self._threads):
            self.abort()
        for e in self._encs:
            e.close()


def slice_rows(height: int, n: int):
    """CTU rows of n full-width slices of a picture `height` high: as even as whole rows allow, the taller ones first."""
    rows = (height + 31) // 32
    n = max(1, min(n, rows, 16))
    return [rows // n + (1 if k < rows % n else 0) for k in range(n)]


class SlicedEncoder:
    """One PICTURE over several MI355X (BASELINE configs[4]): the picture is cut into full-width bands of CTU rows, band k is coded by its own
    session on devices[k] as one slice (own CABAC stream, slice_segment_address in its header), and the slices of a picture are put together
    into one access unit.  halo=True (default): the sessions exchange rows per picture (include/mihevc.h slice_halo; SURVEY §8e's neighbour halo:
    point-to-point pulls over xGMI, no collective) — the reference rows either side of every seam, so motion vectors cross seams as in a whole
    picture, and the pre-deblock rows + CU records, so deblocking and SAO run across the seams; the rate controller plans the whole picture from
    inputs summed over the bands.  halo=False: nothing is exchanged (motion-constrained slices, filters stop at the seams, one rate controller
    per band: round 2's form, -1.5 dB at 4320p over 8).  `devices` may name a device several times (tests: all bands on one GPU)."""

    _group_ids = iter(range(1, 1 << 30))

    def __init__(self, cfg: _lib.Config, devices, keep_recon: bool = False, halo: bool = True):
        import queue
        self.cfg, self.devices = cfg, list(devices)
        self.rows = slice_rows(cfg.height, len(self.devices))
        self.devices = self.devices[:len(self.rows)]
        self.halo = bool(halo) and len(self.rows) > 1
        group = next(SlicedEncoder._group_ids) if self.halo else 0
        self._bands, self._cfgs, y0 = [], [], 0
        for k, r in enumerate(self.rows):
            c = type(cfg).from_buffer_copy(bytes(cfg))
            y1 = min(cfg.height, y0 + 32 * r)
            c.pic_height, c.slice_count, c.slice_index, c.height = cfg.height, len(self.rows), k, y1 - y0
            for i, rr in enumerate(self.rows):
                c.slice_ctu_rows[i] = rr
            c.rate_share_q16 = max(1, round(65536 * r / sum(self.rows)))
            c.slice_halo, c.slice_group = int(self.halo), group
            self._cfgs.append(c)
            self._bands.append((y0, y1))
            y0 = y1
        self._encs = []
        try:
            for c, d in zip(self._cfgs, self.devices):
                self._encs.append(Encoder(c, device=d, keep_recon=keep_recon))
        except Exception:
            for e in self._encs:
                e.close()
            raise
        self._q = [queue.Queue(maxsize=8) for _ in self._encs]
        self._out = [dict() for _ in self._encs]            # per slice: pts -> (data, key)
        self._lock = threading.Lock()
        self._err = []
        self._aborted = False
        self._threads = [threading.Thread(target=self._worker, args=(k,), daemon=True) for k in range(len(self._encs))]
        for t in self._threads:
            t.start()
        self._n_in, self._next_out = 0, 0

    def _worker(self, k):
        enc, q = self._encs[k], self._q[k]
        try:
            while True:
                item = q.get()
                if item is None:
                    break
                y, u, v, pts = item
                enc.send(y, u, v, pts=pts)
                self._collect(k)
            if not self._aborted:
                enc.flush()
                self._collect(k)
        except Exception as exc:
            self._err.append(exc)
            for e in self._encs:                    # the other bands may be waiting for this one inside a native call: let them go
                e.abort()

    def _collect(self, k):
        got = list(self._encs[k].packets())
        if got:
            with self._lock:
                for data, pts, key in got:
                    self._out[k][pts] = (data, key)

    def send(self, y, u, v):
        import queue
        for k, (y0, y1) in enumerate(self._bands):
            item = (y[y0:y1], u[y0 // 2:y1 // 2], v[y0 // 2:y1 // 2], self._n_in)
            while True:
                if self._err:
                    raise self._err[0]
                try:
                    self._q[k].put(item, timeout=0.2)
                    break
                except queue.Full:
                    continue
        self._n_in += 1

    def ready(self):
        """Access units that are complete (every slice present) and next in order: (data, pts, key)."""
        out = []
        with self._lock:
            while all(self._next_out in o for o in self._out):
                parts = [o.pop(self._next_out) for o in self._out]
                out.append((b"".join(p[0] for p in parts), self._next_out, parts[0][1]))
                self._next_out += 1
        return out

    _stop_workers = ShardedEncoder._stop_workers

    def finish(self):
        self._stop_workers(drain=False)
        if self._err:
            raise self._err[0]
        return self.ready()

    def abort(self):
        self._aborted = True
        for e in self._encs:                        # a band blocked in a native call waiting for its neighbours returns with an error
            e.abort()
        self._stop_workers(drain=True)

    def headers(self) -> bytes:
        return self._encs[0].headers()

    def stats(self):
        return [e.stats() for e in self._encs]

    def recon(self, index: int):
        """the picture's reconstruction: the bands' reconstructions stacked (sessions opened with keep_recon)"""
        parts = [e.recon(index) for e in self._encs]
        return tuple(np.vstack([p[i] for p in parts]) for i in range(3))

    def close(self):
        if any(t.is_alive() for t in self._threads):
            self.abort()
        for e in self._encs:
            e.close()


def upscale_target(w: int, h: int, target_height: int = 0) -> Tuple[int, int]:
    """The size the reference's upscaling tool gives a w x h clip: target_height 0 picks 1080 lines below 1080, 2160 below 2160, else the source's own height; a
    non-zero target_height is taken as given.  scale = target_height / h and width = int(w * scale), in its floating-point arithmetic, the width then lowered to
    the next even number (4:2:0)."""
    if target_height == 0:
        target_height = 1080 if h < 1080 else 2160 if h < 2160 else h
    scale = target_height / h
    return int(w * scale) & ~1, int(target_height)


def sr_target_size(sw: int, sh: int, scale: int, target=None) -> Tuple[int, int]:
    """The session size of a sw x sh source through a model of `scale` (Encoder.send_sr_yuv, Encoder.send_sr_fit).  target None: the network's own output,
    (scale sw, scale sh).  'auto': upscale_target(sw, sh, 0), the reference's rule (1080 lines for sources below 1080, 2160 below 2160); an int: that height,
    upscale_target(sw, sh, height); a (w, h) tuple is taken as given.  The result must be the network's output size, or a reduction of it the device scaler
    takes: all sizes even and at least 16, per axis between a quarter of the network's output and that output.  ValueError names the sizes otherwise; a target
    LARGER than the network's output (a 240-line source to 1080 through a x4 model) is one of them."""
    sw, sh, scale = int(sw), int(sh), int(scale)
    nw, nh = scale * sw, scale * sh
    if target is None:
        return nw, nh
    if isinstance(target, str):
        if target != 'auto':
            raise ValueError(f"sr_target={target!r} takes (w, h), a height or 'auto'")
        w, h = upscale_target(sw, sh, 0)
    elif isinstance(target, int) and not isinstance(target, bool):
        if target < 1:
            raise ValueError(f"sr_target={target!r} takes (w, h), a height or 'auto'")
        w, h = upscale_target(sw, sh, target)
    else:
        try:
            w, h = (int(x) for x in target)
        except (TypeError, ValueError):
            raise ValueError(f"sr_target={target!r} takes (w, h), a height or 'auto'") from None
    if (w, h) == (nw, nh):
        return w, h
    if any(x % 2 or x < 16 for x in (w, h, nw, nh)) or not nw <= 4 * w <= 4 * nw or not nh <= 4 * h <= 4 * nh:
        raise ValueError(f"a {sw}x{sh} source through a x{scale} model is {nw}x{nh}: {w}x{h} is not that size or an even reduction of it by at most 4 per axis")
    return w, h


def remux_audio(video_mp4: Path, source: Path, out_path: Path, info: VideoInfo) -> bool:
    """The native path writes video only; the reference always carries the source's audio as AAC (core/transcoder.py:423-450,480-489).
    When the source has audio (only container inputs can, and those need ffmpeg to be decoded at all) the video track is copied and the
    audio encoded with the reference's own flags.  False when ffmpeg is missing or fails: the caller then falls down the ladder."""
    import shutil
    import subprocess
    from .transcoder import VIDEO_METADATA_FLAGS, get_audio_flags
    if shutil.which('ffmpeg') is None:
        return False
    cmd = ['ffmpeg', '-hide_banner', '-y', '-i', str(video_mp4), '-i', str(source), '-map', '0:v:0', '-map', '1:a:0?', '-map_metadata', '1',
           '-c:v', 'copy', '-tag:v', 'hvc1'] + VIDEO_METADATA_FLAGS
    for kv in ('handler_name=SoundHandler', f'language={info.audio_language or "eng"}', 'title="Main Audio"'):
        cmd += ['-metadata:s:a:0', kv]
    cmd += get_audio_flags(info.audio_channels) + ['-brand', 'mp42', '-movflags', '+write_colr+use_metadata_tags+faststart', str(out_path)]
    try:
        return subprocess.run(cmd, capture_output=True).returncode == 0 and Path(out_path).exists()
    except Exception:
        return False


def _parse_upscale(upscale, sw: int, sh: int) -> Tuple[int, int]:
    """upscale= of encode_file: (w, h), a target height, or 'auto' for upscale_target's rule -> the target size.  ValueError / TypeError / IndexError otherwise"""
    if isinstance(upscale, str):
        if upscale != 'auto':
            raise ValueError(upscale)
        return upscale_target(sw, sh, 0)
    if isinstance(upscale, int) and not isinstance(upscale, bool):
        if upscale < 1:
            raise ValueError(upscale)
        return upscale_target(sw, sh, upscale)
    target = (int(upscale[0]), int(upscale[1]))
    if len(upscale) != 2:
        raise ValueError(upscale)
    return target


def _load_sr(sr_model, sr_denoise):
    """sr_model= / sr_denoise= of encode_file -> an hevc_amd.sr.RrdbNet or CompactNet: a model as it is, a path or state dict loaded, a pair blended by
    sr_denoise.  Raises what the loaders raise, and ValueError for a pair without its strength or a strength without its pair"""
    from . import sr as sr_mod
    one = lambda m: m if isinstance(m, (sr_mod.RrdbNet, sr_mod.CompactNet)) else sr_mod.load_model(m)
    if isinstance(sr_model, (tuple, list)):
        if len(sr_model) != 2 or sr_denoise is None or isinstance(sr_denoise, bool):
            raise ValueError("a pair (model, denoise partner) goes with sr_denoise = 0 .. 1")
        return sr_mod.blend(one(sr_model[0]), one(sr_model[1]), sr_denoise)
    if sr_denoise is not None:
        raise ValueError("sr_denoise= goes with a pair (model, denoise partner) of compact models")
    return one(sr_model)


def _field_order(file_path: Path, tff, deinterlace: str):
    """the field order of deinterlace=: tff when given, else the y4m header's It / Ib tag or ffprobe's field_order; a source that names none is top field first,
    but for 'auto', which then does nothing (None)"""
    from . import yuvio
    order = tff
    if order is None:
        suffix = Path(file_path).suffix.lower()
        if suffix == '.y4m':
            probe_clip = yuvio.open_clip(Path(file_path))
            order = {'t': True, 'b': False}.get(probe_clip.interlace)
            probe_clip.close()
        elif suffix != '.yuv':
            from .probe import probe_field_order
            order = probe_field_order(Path(file_path))
        if order is None and deinterlace != 'auto':
            order = True
    return order


def _sr_source_colour(info: VideoInfo, clip, height: int):
    """(matrix, full range) of a Y'CbCr source on its way into the network: the probed matrix, BT.601 below 720 lines and BT.709 from there on when the probe does
    not know it; yuvj* files read directly are full range (the pipe hands yuvj* over as limited range)"""
    from . import yuvio
    matrix = _COLOUR_CODES["matrix"].get(info.color_space, 0)
    if matrix not in (1, 5, 6, 9):
        matrix = 6 if height < 720 else 1
    return matrix, (info.pix_fmt or '').lower().startswith('yuvj') and not isinstance(clip, yuvio._PipeClip)


def _carry_audio(wants_audio: bool, video_path: Path, file_path: Path, out_path: Path, info: VideoInfo) -> bool:
    """the end of an encode, the video track written: a source with audio gets its audio carried over.  False: the remux failed"""
    if not wants_audio:
        return True
    good = remux_audio(video_path, Path(file_path), Path(out_path), info)
    try:
        video_path.unlink()
    except OSError:
        pass
    if not good:
        logger.warning("%s: audio could not be carried over (ffmpeg remux failed); falling back to the ffmpeg path", Path(file_path).name)
    return good


CHAIN_KEYS = ("deinterlace", "tff", "denoise", "size", "upscale", "sr_model", "sr_target", "sr_denoise", "sharpen", "antiring", "interpolate", "interp_mode")


def _encode_file_chain(file_path: Path, out_path: Path, info: VideoInfo, progress_callback, total_frames: int, stop_event, device, chain) -> int:
    """encode_file(chain=...): the options of the dict become one _lib.Chain, the session opens at what mihevc_chain_plan_for says of it, every frame goes through
    Encoder.send_chain.  Everything is judged before the session is opened"""
    import copy
    from fractions import Fraction
    from . import mp4, yuvio
    from .transcoder import calculate_apple_hevc_level, calculate_dynamic_values
    name = Path(file_path).name
    if not isinstance(chain, dict) or set(chain) - set(CHAIN_KEYS):
        logger.error("%s: chain= takes a dict with keys out of %s", name, ", ".join(CHAIN_KEYS))
        return 1
    opt = {k: chain.get(k) for k in CHAIN_KEYS}
    sw0, sh0 = int(info.width), int(info.height)
    kw = {}
    # field
    deinterlace = opt["deinterlace"]
    if deinterlace is not None:
        if deinterlace not in ('frame', 'field', 'auto', 'ivtc', 'match'):
            logger.error("%s: chain: deinterlace=%r takes 'frame', 'field', 'auto', 'ivtc' or 'match'", name, deinterlace)
            return 1
        order = _field_order(file_path, opt["tff"], deinterlace)
        if deinterlace in ('ivtc', 'match'):
            kw.update(field="fieldmatch", tff=bool(order), decimate=deinterlace == 'ivtc', fm_deint=True)
        elif order is not None:
            kw.update(field="deint", tff=bool(order), field_rate=deinterlace == 'field')
    elif opt["tff"] is not None:
        logger.error("%s: chain: tff= goes with deinterlace=", name)
        return 1
    # denoise
    dn = opt["denoise"]
    if dn is not None and not (isinstance(dn, int) and not isinstance(dn, bool) and dn == 0):
        try:
            kw["denoise"] = _lib.denoise_strength(dn)
        except (TypeError, ValueError):
            logger.error("%s: chain: denoise=%r takes a level 0 .. 3 or four thresholds 0 .. 255", name, dn)
            return 1
    # resize
    if sum(opt[k] is not None for k in ("size", "upscale", "sr_model")) > 1:
        logger.error("%s: chain: one of size=, upscale=, sr_model=", name)
        return 1
    target, sr = (sw0, sh0), None
    sharpen, antiring = (8 if opt[k] is None else opt[k] for k in ("sharpen", "antiring"))
    if opt["upscale"] is None and (opt["sharpen"] is not None or opt["antiring"] is not None):
        logger.error("%s: chain: sharpen= and antiring= go with upscale=", name)
        return 1
    if opt["sr_model"] is None and (opt["sr_target"] is not None or opt["sr_denoise"] is not None):
        logger.error("%s: chain: sr_target= and sr_denoise= go with sr_model=", name)
        return 1
    try:
        if opt["size"] is not None:
            target = (int(opt["size"][0]), int(opt["size"][1]))
            if len(opt["size"]) != 2:
                raise ValueError(opt["size"])
            kw["resize"] = "scale"
        elif opt["upscale"] is not None:
            if any(isinstance(x, bool) or not isinstance(x, int) for x in (sharpen, antiring)):
                raise ValueError("sharpen / antiring")
            target = _parse_upscale(opt["upscale"], sw0, sh0)
            kw.update(resize="upscale", sharpen=sharpen, antiring=antiring)
        elif opt["sr_model"] is not None:
            sr = _load_sr(opt["sr_model"], opt["sr_denoise"])
            target = sr_target_size(sw0, sh0, sr.scale, opt["sr_target"])
            kw["resize"] = "sr"
    except (OSError, ValueError, TypeError, RuntimeError, KeyError, IndexError) as e:
        logger.error("%s: chain: the resize stage: %s", name, e)
        return 1
    # interpolate
    if opt["interpolate"] is not None:
        kw.update(interpolate=opt["interpolate"], interp_mode='mc' if opt["interp_mode"] is None else opt["interp_mode"])
    elif opt["interp_mode"] is not None:
        logger.error("%s: chain: interp_mode= goes with interpolate=", name)
        return 1
    clip = yuvio.open_any(Path(file_path), info, native_formats=True, rgb_formats=False)
    mux = None
    ok = False
    try:
        fmt = getattr(clip, 'src_format', None)
        planar420 = getattr(clip, 'rgb_format', None) is None and (fmt is None or (fmt.chroma == 420 and not fmt.semi_planar and not fmt.msb_aligned))
        src_depth = int(fmt.bit_depth) if fmt is not None else int(clip.bit_depth)
        if not planar420 or src_depth not in (8, 10):
            logger.error("%s: chain= takes a planar 4:2:0 source at 8 or 10 bit (%r)", name, fmt)
            return 1
        sw, sh = int(clip.width), int(clip.height)
        out_info = copy.copy(info)
        out_info.width, out_info.height = int(target[0]), int(target[1])
        if src_depth > 8 and bit_depth_of(out_info) == 8:      # the file's own header outranks the probe, as in encode_file
            out_info.pix_fmt = 'yuv420p10le'
        depth = bit_depth_of(out_info)
        if sr is not None:
            sr_matrix, sr_full = _sr_source_colour(info, clip, sh)
            kw.update(sr_matrix=sr_matrix, sr_full_range=sr_full)
        try:
            c = _lib.chain(sw, sh, src_depth, **kw)
        except (TypeError, ValueError) as e:
            logger.error("%s: chain: %s", name, e)
            return 1
        n_src = clip.n_frames or total_frames
        matrix = _COLOUR_CODES["matrix"].get(out_info.color_space, 0)
        if sr is not None and matrix not in (1, 5, 6, 9):
            matrix = sr_matrix
        plan = _lib.chain_plan(c, out_info.width, out_info.height, depth, matrix if sr is not None else 1, sr.scale if sr is not None else 0, int(n_src or 0))
        if plan is None:
            logger.error("%s: chain: %r in front of a %dx%d session at %d bit is not a chain the device takes (no stage on, a size, ratio or strength out of range)",
                         name, c, out_info.width, out_info.height, depth)
            return 1
        rate = Fraction(plan.rate_num, plan.rate_den)
        exact = Fraction(str(info.fps or 30.0)).limit_denominator(1001) * rate
        out_info.fps = float(info.fps or 30.0) * float(rate) if rate.denominator == 1 else float(exact)
        nb = int(getattr(info, 'nb_frames', 0) or 0)
        out_info.nb_frames = int(_lib.chain_plan(c, out_info.width, out_info.height, depth, matrix if sr is not None else 1, sr.scale if sr is not None else 0, nb).pictures)
        crf, _cq, maxrate, bufsize, gop = calculate_dynamic_values(out_info)
        level, tier = calculate_apple_hevc_level(out_info)
        cfg = config_for(out_info, crf, maxrate, bufsize, gop, level, tier)
        if rate.denominator != 1:
            cfg.fps_num, cfg.fps_den = exact.numerator, exact.denominator
        if sr is not None and cfg.matrix not in (1, 5, 6, 9):
            cfg.matrix = sr_matrix
        total = int(plan.pictures)
        wants_audio = bool(info.audio_channels and info.audio_channels > 0) and Path(file_path).suffix.lower() not in ('.y4m', '.yuv')
        video_path = Path(out_path).with_suffix('.video.mp4') if wants_audio else Path(out_path)
        mux = mp4.Mp4Writer(video_path, cfg)
        n_out = 0

        def progress():
            if progress_callback:
                try:
                    progress_callback(name, n_out, total)
                except Exception:
                    logger.debug("progress_callback raised", exc_info=True)

        with Encoder(cfg, device=device or 0) as enc:
            if sr is not None:
                enc.set_sr_model(sr)
            enc.set_chain(sw, sh, src_depth, chain=c)
            for i, planes in enumerate(clip.frames()):
                if stop_event is not None and stop_event.is_set():
                    return 1
                enc.send_chain(*planes, pts=i)
                for data, pts, key, dts in enc.packets_dts():
                    mux.add_sample(data, pts, key, dts)
                    n_out += 1
                progress()
            enc.flush()
            for data, pts, key, dts in enc.packets_dts():
                mux.add_sample(data, pts, key, dts)
                n_out += 1
            progress()
            headers = enc.headers()
        if n_out == 0:
            return 1
        mux.finish(headers)
        mux = None
        if not _carry_audio(wants_audio, video_path, file_path, out_path, out_info):
            return 1
        ok = True
        return 0
    finally:
        if mux is not None and not ok:
            mux.abort()
        clip.close()


def encode_file(file_path: Path, out_path: Path, info: VideoInfo, progress_callback: Optional[Callable[[str, int, int], None]] = None,
                total_frames: int = 1, stop_event: Optional[threading.Event] = None, device: Optional[int] = None, debug: bool = False,
                devices=None, row_split: bool = False, native_rgb: bool = False, size=None, deinterlace: Optional[str] = None,
                tff: Optional[bool] = None, denoise=None, lut=None, lut_bit_depth: int = 8, interpolate: Optional[int] = None, interp_mode: str = 'mc',
                upscale=None, sharpen: int = 8, antiring: int = 8, sr_model=None, sr_target=None, sr_denoise=None, chain: Optional[dict] = None) -> int:
    """Encode `file_path` to `out_path` (MP4/hvc1) on an MI355X.  Returns 0 on success, 1 on failure/cancel —
    the same (returncode) shape `run_ffmpeg` gives `convert_video` (core/transcoder.py:497-535).  native_rgb: a container probed as one of the RGB pixel
    formats of _lib.rgb_format_for is decoded to that format and converted on the device (Encoder.send_rgb) instead of by swscale; the session signals the
    probed matrix, BT.709 when that is `gbr` or unknown.  size=(w, h): the session, its level and the MP4 track take this size and every picture of the source,
    delivered at its own size, is scaled down on the device (Encoder.send_scaled): planar 4:2:0 sources on one device only, per axis at most 4:1.
    deinterlace: the source's frames are woven interlaced frames, deinterlaced on the device (Encoder.send_deint).  'frame': one picture per
    frame; 'field': one per field, so the session, its level, the rate figures and the MP4 track run at twice the frame rate; 'auto': 'frame' when the source
    says it is interlaced (the y4m header's It / Ib tag, else ffprobe's field_order), nothing otherwise.  tff: the field order, None to take the source's word
    (top field first when it has none).  Planar 4:2:0 sources at the session's depth on one device; not together with size= or native_rgb.  'ivtc' and 'match':
    the frames carry film in fields (3:2 pulldown) and go through inverse telecine instead (Encoder.send_fieldmatch), with the same exclusions and
    field-order lookup: 'ivtc' matches fields and drops one frame of every five, so the session, its level, the progress total and the MP4 track run at exactly
    4/5 of the source rate (30000/1001 gives 24000/1001); 'match' only matches fields and keeps the rate.  'auto' keeps meaning the deinterlacer.
    denoise: a level 1 .. 3 or a tuple of four thresholds (Encoder.send_denoise): every frame is denoised on the device in front of the session.
    None and 0: nothing changes.  Planar 4:2:0 sources at the session's depth on one device; not together with deinterlace=, size=, native_rgb, sliced sessions or several devices.
    lut: every frame goes through a 3D colour table on the device (Encoder.send_lut3d): the path of a .cube file, an (n, n, n, 3) array, or
    'hdr-to-sdr' for the built-in table of lut3d.hdr_to_sdr (the transfer from the probe, PQ unless it says HLG; peak_nits from the probed master_display when
    there is one).  The session opens as SDR whatever the probe says of the source: 8 bit (lut_bit_depth=10: Main10), colour description 1/1/1, no HDR10 SEI, the
    level and tier of an SDR clip; the reader keeps delivering the source's own planar 4:2:0 frames at 8, 10 or 12 bit, and the source's matrix is the probed one
    (BT.2020 for HDR, else BT.709 when unknown).  One device; not together with size=, native_rgb, deinterlace= or denoise=.
    interpolate: 2, 3 or 4: the frame rate is multiplied on the device (Encoder.send_interpolate), interp_mode 'mc' by motion-compensated
    interpolation, 'blend' by blending; the session, its level, the rate figures and the MP4 track run at that multiple of the probed rate, n frames give
    interpolate * (n - 1) + 1 pictures, and the progress total counts pictures.  None: nothing changes.  Planar 4:2:0 sources at the session's depth on one
    device; not together with size=, native_rgb, deinterlace=, denoise= or lut=.
    upscale: (w, h), a target height, or 'auto' for upscale_target's rule: the session, its level and the MP4 track take that size and every picture of the
    source, delivered at its own size, is enlarged on the device (Encoder.send_upscaled) with sharpen (0 .. 64 sixteenths) and antiring (0 .. 8
    eighths).  None: nothing changes.  Planar 4:2:0 sources on one device, per axis between 1:1 and 1:4; not together with size=, native_rgb, deinterlace=,
    denoise=, lut=, interpolate=, sliced sessions or several devices.
    sr_model: the path of an RRDBNet or SRVGGNetCompact .pth file, a state dict, or an hevc_amd.sr.RrdbNet / CompactNet (hevc_amd.sr.load_model chooses by
    the keys): every picture is enlarged by the network on the device.  A pair (model, denoise partner) of compact models with
    sr_denoise = 0 .. 1 is the compact family's denoise strength (realesr-general-x4v3 with realesr-general-wdn-x4v3): the two are blended on the host
    (hevc_amd.sr.blend), sr_denoise being the weight of the FIRST model.  The reference's tool has a noise level 0 .. 3 and states no mapping of it onto this
    strength, so none is made up here: the caller gives the strength.  sr_denoise with a single model or an RRDBNet, or a pair without it, is an error.  A
    compact model of scale 2 takes odd R'G'B' source sides.  A container that probes as one of the RGB pixel formats is asked for as it is, as native_rgb=True asks (Encoder.send_sr).  A planar 4:2:0
    Y'CbCr container at 8, 10 or 12 bit is read in its own format and brought to R'G'B' on the device (Encoder.send_sr_yuv): its matrix is the probed one, and
    when the probe does not know it BT.601 below 720 lines and BT.709 from there on, which is what players and swscale assume; its range is the probed one
    (yuvj* files read directly are full range; the pipe hands yuvj* over as limited range).  Any other format (4:2:2, 4:4:4, semi-planar) is refused by name.
    sr_target: None: the session, its level and the MP4 track open at scale x the source size.  'auto', a height or (w, h) (sr_target_size): they open at that
    size and the network's picture is scaled down to it on the device; 'auto' is what the reference's restoration tool does.  sr_target without sr_model is
    refused.  One device; not together with any other source filter, size= or upscale=.  There is no tiling: a frame the device cannot hold ends the run.
    chain: a dict of the options above that go TOGETHER (Encoder.set_chain / send_chain): deinterlace= and tff=, denoise=, one of size= | upscale=
    (sharpen=, antiring=) | sr_model= (sr_target=, sr_denoise=), interpolate= and interp_mode=, each meaning what the option of that name means; the filters run
    in that fixed order on the device, field and denoise at the source's size, interpolation at the session's.  The session's size, level, rate figures, the
    progress total and the MP4 track follow the chain's size and rate (hevc_amd/csrc/chain_plan.h); 'ivtc' sets the rate as an exact fraction.  Planar 4:2:0
    sources at 8 or 10 bit on one device; chain= together with any of those options outside the dict, with native_rgb, lut= or several devices is refused.
    chain=dict(denoise=n, sr_model=p, sr_target='auto', interpolate=k) is the whole process_video of the reference's restoration tool on the device."""
    if chain is not None:
        if (size is not None or deinterlace is not None or tff is not None or denoise is not None or lut is not None or interpolate is not None or upscale is not None
                or sr_model is not None or sr_target is not None or sr_denoise is not None or native_rgb or row_split or (devices and len(devices) > 1)):
            logger.error("%s: chain= takes its filters inside the dict, one device, and none of native_rgb, lut=", Path(file_path).name)
            return 1
        return _encode_file_chain(file_path, out_path, info, progress_callback, total_frames, stop_event, device, chain)
    import copy
    from . import mp4, yuvio
    from .transcoder import calculate_apple_hevc_level, calculate_dynamic_values

    if denoise is not None and not (isinstance(denoise, int) and not isinstance(denoise, bool) and denoise == 0):
        try:
            denoise, bad = _lib.denoise_strength(denoise), False
        except (TypeError, ValueError):
            bad = True
        if bad or deinterlace is not None or size is not None or native_rgb or (devices and len(devices) > 1):      # (several devices: sharded or sliced)
            logger.error("%s: denoise=%r takes a level 0 .. 3 or four thresholds 0 .. 255, one device, and none of deinterlace=, size=, native_rgb",
                         Path(file_path).name, denoise)
            return 1
    else:
        denoise = None
    if upscale is not None:
        sw0, sh0 = int(info.width), int(info.height)
        if (size is not None or native_rgb or deinterlace is not None or denoise is not None or lut is not None or interpolate is not None or (devices and len(devices) > 1)
                or isinstance(sharpen, bool) or not isinstance(sharpen, int) or not 0 <= sharpen <= 64 or isinstance(antiring, bool) or not isinstance(antiring, int)
                or not 0 <= antiring <= 8):
            logger.error("%s: upscale=%r takes (w, h), a height or 'auto', sharpen 0 .. 64, antiring 0 .. 8, one device, and none of size=, native_rgb, deinterlace=, "
                         "denoise=, lut=, interpolate=", Path(file_path).name, upscale)
            return 1
        try:
            target = _parse_upscale(upscale, sw0, sh0)
        except (TypeError, ValueError, IndexError):
            logger.error("%s: upscale=%r takes (w, h), a height or 'auto'", Path(file_path).name, upscale)
            return 1
        if (target[0] % 2 or target[1] % 2 or sw0 % 2 or sh0 % 2 or min(sw0, sh0) < 16 or not sw0 <= target[0] <= 4 * sw0 or not sh0 <= target[1] <= 4 * sh0):
            logger.error("%s: upscale=%r: %dx%d to %dx%d is not an enlargement of even sizes by 1 .. 4 per axis", Path(file_path).name, upscale, sw0, sh0, target[0], target[1])
            return 1
        upscale, size = target, target      # from here on the road of size=: the session takes the target, the clip is opened at the source's own size
    else:
        upscale = None
    sr = None
    if sr_model is not None:
        if (size is not None or deinterlace is not None or denoise is not None or lut is not None or interpolate is not None or (devices and len(devices) > 1)):
            logger.error("%s: sr_model= takes one device and none of size=, upscale=, deinterlace=, denoise=, lut=, interpolate=", Path(file_path).name)
            return 1
        try:
            sr = _load_sr(sr_model, sr_denoise)
        except (OSError, ValueError, TypeError, RuntimeError, KeyError) as e:
            logger.error("%s: sr_model: %s", Path(file_path).name, e)
            return 1
        sw0, sh0 = int(info.width), int(info.height)
        if min(sw0, sh0) < 4 or (sr.scale == 2 and not hasattr(sr, "convs") and (sw0 % 2 or sh0 % 2)):
            logger.error("%s: sr_model: a %dx%d source does not fit a scale %d model", Path(file_path).name, sw0, sh0, sr.scale)
            return 1
        sr_name = (info.pix_fmt or '').lower()
        sr_yuv = _lib.rgb_format_for(sr_name) is None      # a Y'CbCr container: read in its own format, converted in front of the network
        if sr_yuv:
            yf = _lib.src_format_for('yuv' + sr_name[4:] if sr_name.startswith('yuvj') else sr_name)
            if yf is None or yf.chroma != 420 or yf.semi_planar or yf.msb_aligned or yf.bit_depth not in (8, 10, 12) or sw0 % 2 or sh0 % 2:
                logger.error("%s: sr_model= takes an R'G'B' source or a planar 4:2:0 Y'CbCr source at 8, 10 or 12 bit with even sides (%r, %dx%d)",
                             Path(file_path).name, info.pix_fmt, sw0, sh0)
                return 1
        try:
            sr_size = sr_target_size(sw0, sh0, sr.scale, sr_target)
        except ValueError as e:
            logger.error("%s: %s", Path(file_path).name, e)
            return 1
        native_rgb, size = not sr_yuv, sr_size      # the road of size=: the session takes the target, the clip is opened at the source's own size
    elif sr_target is not None:
        logger.error("%s: sr_target= goes with sr_model=", Path(file_path).name)
        return 1
    elif sr_denoise is not None:
        logger.error("%s: sr_denoise= goes with sr_model=", Path(file_path).name)
        return 1
    clip_info = info        # what the clip is opened with: the source's own description, rate and frame count
    if interpolate is not None:
        if (isinstance(interpolate, bool) or not isinstance(interpolate, int) or interpolate not in (2, 3, 4) or interp_mode not in _lib.INTERP_MODES or denoise is not None
                or lut is not None or deinterlace is not None or size is not None or native_rgb or (devices and len(devices) > 1)):
            logger.error("%s: interpolate=%r takes 2, 3 or 4, interp_mode 'mc' or 'blend', one device, and none of size=, native_rgb, deinterlace=, denoise=, lut=",
                         Path(file_path).name, interpolate)
            return 1
        info = copy.copy(info)      # the session, its level and the track run at the multiplied rate
        info.fps = float(info.fps or 30.0) * interpolate
        info.nb_frames = max((int(getattr(info, 'nb_frames', 0) or 0) - 1) * interpolate + 1, 0)
    lut_table = None        # the uint16 table once lut= is on
    if lut is not None:
        from . import lut3d
        if denoise is not None or deinterlace is not None or size is not None or native_rgb or (devices and len(devices) > 1) or lut_bit_depth not in (8, 10):
            logger.error("%s: lut= takes a .cube path, an (n, n, n, 3) table or 'hdr-to-sdr', lut_bit_depth 8 or 10, one device, and none of size=, native_rgb, "
                         "deinterlace=, denoise=", Path(file_path).name)
            return 1
        try:
            if isinstance(lut, str) and lut == 'hdr-to-sdr':
                from .utils import parse_master_display
                transfer = 'hlg' if (info.color_transfer or '').lower() == 'arib-std-b67' else 'pq'
                peak = parse_master_display(info.master_display).lum[0] / 10000.0 if (info.master_display or '').strip() else 1000.0
                lut_table = lut3d.hdr_to_sdr(65, transfer, min(max(peak, lut3d.SDR_PEAK_NITS), 10000.0))
            elif isinstance(lut, (str, Path)):
                lut_table = lut3d.quantise(lut3d.read_cube(lut))
            else:
                lut_table = lut3d.as_uint16(lut)
        except (OSError, TypeError, ValueError) as e:
            logger.error("%s: lut=%r: %s", Path(file_path).name, lut if isinstance(lut, (str, Path)) else type(lut).__name__, e)
            return 1
        lut_src_matrix = _COLOUR_CODES["matrix"].get(info.color_space, 9 if info.hdr else 1)
        lut_src_full = (info.pix_fmt or '').lower().startswith('yuvj')
        info = copy.copy(info)      # the session, its level and the track are those of an SDR clip
        info.hdr, info.master_display, info.max_cll = False, '', ''
        info.color_primaries = info.color_transfer = info.color_space = 'bt709'
        info.pix_fmt = 'yuv420p10le' if lut_bit_depth == 10 else 'yuv420p'
    deint = None            # (top field first, field rate) once deinterlacing is on
    ivtc = None             # (top field first, decimate) once inverse telecine is on
    ivtc_rate = None        # 'ivtc': the session's rate, 4/5 of the source's as a fraction
    if deinterlace is not None:
        if deinterlace not in ('frame', 'field', 'auto', 'ivtc', 'match') or size is not None or native_rgb or (devices and len(devices) > 1):
            logger.error("%s: deinterlace=%r takes 'frame', 'field', 'auto', 'ivtc' or 'match', one device, and neither size= nor native_rgb", Path(file_path).name, deinterlace)
            return 1
        order = _field_order(file_path, tff, deinterlace)
        if deinterlace in ('ivtc', 'match'):
            ivtc = (bool(order), deinterlace == 'ivtc')
            if ivtc[1]:
                from fractions import Fraction
                ivtc_rate = Fraction(str(info.fps or 30.0)).limit_denominator(1001) * Fraction(4, 5)
                info = copy.copy(info)
                info.fps = float(ivtc_rate)
                info.nb_frames = int(getattr(info, 'nb_frames', 0) or 0) * 4 // 5
        elif order is not None:
            deint = (bool(order), deinterlace == 'field')
        if deint and deint[1]:
            info = copy.copy(info)
            info.fps = float(info.fps or 30.0) * 2
            info.nb_frames = int(getattr(info, 'nb_frames', 0) or 0) * 2
    src_size = (int(info.width), int(info.height))
    if size is not None:        # rate, level and track follow the coded size; the clip below is still opened at the source's own
        src_info, info = info, copy.copy(info)
        info.width, info.height = int(size[0]), int(size[1])
    crf, _cq, maxrate, bufsize, gop = calculate_dynamic_values(info)
    level, tier = calculate_apple_hevc_level(info)
    sliced = bool(row_split and devices and len(devices) > 1)      # SlicedEncoder takes planar 4:2:0 only
    clip = yuvio.open_any(Path(file_path), (clip_info if deint or ivtc or lut_table is not None or interpolate is not None else info) if size is None else src_info, native_formats=not sliced, rgb_formats=native_rgb and not sliced)
    mux = None
    ok = False
    try:
        if lut_table is None and clip.bit_depth > 8 and bit_depth_of(info) == 8:      # the file's own header outranks the probe (a y4m tagged C420p10 probed as SDR)
            info.pix_fmt = 'yuv420p10le'
        cfg = config_for(info, crf, maxrate, bufsize, gop, level, tier)
        if ivtc_rate is not None:
            cfg.fps_num, cfg.fps_den = ivtc_rate.numerator, ivtc_rate.denominator
        fmt = getattr(clip, 'src_format', None)     # not the session's own layout: converted on the device (send_fmt)
        rgb = getattr(clip, 'rgb_format', None)     # an RGB source: matrixed and decimated on the device (send_rgb)
        if rgb is not None:
            fmt = rgb
            if cfg.matrix not in (1, 5, 6, 9):
                cfg.matrix = 1
        if lut_table is not None:
            lut_src_depth = int(fmt.bit_depth) if fmt is not None else int(clip.bit_depth)
            planar420 = rgb is None and (fmt is None or (fmt.chroma == 420 and not fmt.semi_planar and not fmt.msb_aligned))
            if not planar420 or lut_src_depth not in (8, 10, 12) or sliced or cfg.width % 2 or cfg.height % 2 or min(cfg.width, cfg.height) < 16:
                logger.error("%s: lut= takes a planar 4:2:0 source at 8, 10 or 12 bit, width and height even (%r, %dx%d)", Path(file_path).name, fmt, cfg.width, cfg.height)
                return 1
            fmt = None
        if sr is not None:
            src_size = (int(clip.width), int(clip.height))
            if sr_yuv:
                planar420 = rgb is None and (fmt is None or (fmt.chroma == 420 and not fmt.semi_planar and not fmt.msb_aligned))
                sr_depth = int(fmt.bit_depth) if fmt is not None else int(clip.bit_depth)
                if not planar420 or sr_depth not in (8, 10, 12) or src_size[0] % 2 or src_size[1] % 2:
                    logger.error("%s: sr_model= takes a planar 4:2:0 Y'CbCr source at 8, 10 or 12 bit with even sides (%r)", Path(file_path).name, fmt)
                    return 1
                sr_matrix, sr_full = _sr_source_colour(info, clip, src_size[1])
                if cfg.matrix not in (1, 5, 6, 9):
                    cfg.matrix = sr_matrix
                fmt = None
            elif rgb is None:
                logger.error("%s: sr_model= takes a source that is read as R'G'B' (%r)", Path(file_path).name, fmt)
                return 1
        elif size is not None:
            fmt420 = fmt is None or (rgb is None and fmt.chroma == 420 and not fmt.semi_planar and not fmt.msb_aligned)
            if not fmt420 or (devices and len(devices) > 1):
                logger.error("%s: %s takes a planar 4:2:0 source on one device (%r)", Path(file_path).name, "size=" if upscale is None else "upscale=", fmt)
                return 1
            src_size = (int(clip.width), int(clip.height))
            src_depth = int(fmt.bit_depth) if fmt is not None else int(clip.bit_depth)
        if fmt is not None and sliced:
            logger.error("%s: a %r source cannot be split by rows", Path(file_path).name, fmt)
            return 1
        if (deint or ivtc) and (fmt is not None or sliced or cfg.width % 2 or cfg.height % 4 or min(cfg.width, cfg.height) < 16):
            logger.error("%s: deinterlace= takes a planar 4:2:0 source at the session's depth, width even, height a multiple of 4 (%r, %dx%d)",
                         Path(file_path).name, fmt, cfg.width, cfg.height)
            return 1
        if denoise is not None and (fmt is not None or cfg.width % 2 or cfg.height % 2 or min(cfg.width, cfg.height) < 16):
            logger.error("%s: denoise= takes a planar 4:2:0 source at the session's depth, width and height even (%r, %dx%d)", Path(file_path).name, fmt, cfg.width, cfg.height)
            return 1
        if interpolate is not None and (fmt is not None or cfg.width % 2 or cfg.height % 2 or min(cfg.width, cfg.height) < 16):
            logger.error("%s: interpolate= takes a planar 4:2:0 source at the session's depth, width and height even (%r, %dx%d)", Path(file_path).name, fmt, cfg.width, cfg.height)
            return 1
        total = (clip.n_frames or total_frames) * (2 if deint and deint[1] else 1)
        if interpolate is not None:
            total = (total - 1) * interpolate + 1
        if ivtc and ivtc[1]:
            total = total * 4 // 5
        wants_audio = bool(info.audio_channels and info.audio_channels > 0) and Path(file_path).suffix.lower() not in ('.y4m', '.yuv')
        video_path = Path(out_path).with_suffix('.video.mp4') if wants_audio else Path(out_path)
        mux = mp4.Mp4Writer(video_path, cfg)
        n_out = 0

        def progress():
            if progress_callback:
                try:
                    progress_callback(Path(file_path).name, n_out, total)
                except Exception:
                    logger.debug("progress_callback raised", exc_info=True)

        if devices and len(devices) > 1:            # one clip over several GPUs: GOP chunks round-robin, or every picture split by CTU rows
            sh = SlicedEncoder(cfg, devices) if row_split else ShardedEncoder(cfg, devices)
            try:
                for planes in clip.frames():
                    if stop_event is not None and stop_event.is_set():
                        return 1
                    y, u, v = (tuple(planes) + (None, None))[:3]
                    if fmt is None:
                        sh.send(y, u, v)
                    else:
                        sh.send(y, u, v, fmt)
                    for data, pts, key in sh.ready():
                        mux.add_sample(data, pts, key)
                        n_out += 1
                    progress()
                for data, pts, key in sh.finish():
                    mux.add_sample(data, pts, key)
                    n_out += 1
                progress()
                headers = sh.headers()
            finally:
                sh.close()                          # joins the workers (abort) before any session is closed
        else:
            with Encoder(cfg, device=device or 0) as enc:
                if lut_table is not None:
                    enc.set_lut3d(lut_table)
                if sr is not None:
                    enc.set_sr_model(sr)
                for i, planes in enumerate(clip.frames()):
                    if stop_event is not None and stop_event.is_set():
                        return 1
                    if sr is not None and sr_yuv:
                        enc.send_sr_yuv(src_size[0], src_size[1], *planes, bit_depth=sr_depth, matrix=sr_matrix, full_range=sr_full, pts=i)
                    elif sr is not None and sr_target is not None:
                        enc.send_sr_fit(fmt, src_size[0], src_size[1], *planes, pts=i)
                    elif sr is not None:
                        enc.send_sr(fmt, src_size[0], src_size[1], *planes, pts=i)
                    elif lut_table is not None:
                        enc.send_lut3d(*planes, bit_depth=lut_src_depth, matrix=lut_src_matrix, full_range=lut_src_full, pts=i)
                    elif deint:
                        enc.send_deint(*planes, tff=deint[0], field_rate=deint[1], pts=i * (2 if deint[1] else 1))
                    elif ivtc:
                        enc.send_fieldmatch(*planes, tff=ivtc[0], decimate=ivtc[1], deint=True, pts=i)
                    elif denoise is not None:
                        enc.send_denoise(*planes, strength=denoise, pts=i)
                    elif interpolate is not None:
                        enc.send_interpolate(*planes, factor=interpolate, mode=interp_mode, pts=i * interpolate)
                    elif upscale is not None:
                        enc.send_upscaled(src_size[0], src_size[1], *planes, bit_depth=src_depth, sharpen=sharpen, antiring=antiring, pts=i)
                    elif size is not None:
                        enc.send_scaled(src_size[0], src_size[1], *planes, bit_depth=src_depth, pts=i)
                    elif fmt is None:
                        enc.send(*planes, pts=i)
                    elif rgb is not None:
                        enc.send_rgb(fmt, *planes, pts=i)
                    else:
                        enc.send_fmt(fmt, *planes, pts=i)
                    for data, pts, key, dts in enc.packets_dts():
                        mux.add_sample(data, pts, key, dts)
                        n_out += 1
                    progress()
                enc.flush()
                for data, pts, key, dts in enc.packets_dts():
                    mux.add_sample(data, pts, key, dts)
                    n_out += 1
                progress()
                headers = enc.headers()
        if n_out == 0:
            return 1
        mux.finish(headers)
        mux = None
        if not _carry_audio(wants_audio, video_path, file_path, out_path, info):
            return 1
        ok = True
        return 0
    finally:
        if mux is not None and not ok:
            mux.abort()                             # cancel, failure or exception: no .mdat.tmp and no open handle stay behind
        clip.close()
