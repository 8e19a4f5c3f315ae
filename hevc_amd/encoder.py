"""Python driver of the native MI355X encoder (C ABI in include/mihevc.h, loaded by hevc_amd._lib).

`Encoder` is a thin object wrapper over one `mihevc_session`; `ShardedEncoder` and `SlicedEncoder` spread one clip over several devices; `config_for` maps
the operating point the reference hands to libx265 (core/transcoder.py:357-412) onto a mihevc_config.  ctypes releases the GIL
during every call, so N worker threads can each drive their own session like the reference's N QThreads each
block on their own ffmpeg child (gui/worker.py:30-52).

`encode_file`, what `convert_video` calls for the 'MI355X' backend, and the rest of the file-level code live in hevc_amd.file_encode; their public names are
re-exported at the end of this module.
"""
from __future__ import annotations

import ctypes as C
import logging
import re
import threading
from fractions import Fraction
from typing import Iterator, Optional, Tuple

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

    def _send_planar(self, who, desc, of, width, height, bit_depth, planes, pts, step, asynchronous, by_ref=True):
        """What the senders of planar 4:2:0 sources share.  who: the sender ('send_scaled': mihevc_send_frame_scaled takes the frame); desc: its descriptor, handed
        to C by reference (by_ref=False: the entry takes none); of: whose size the planes must have, for the message; width, height, bit_depth: of the planes;
        step: how far this frame moves the pts counter."""
        shapes = [(height, width)] + [(height // 2, width // 2)] * 2
        if any(p is None or tuple(p.shape) != s for p, s in zip(planes, shapes)):
            raise ValueError(f"plane shapes {[None if p is None else tuple(p.shape) for p in planes]} do not match {shapes} of {of}")
        es = 1 if bit_depth == 8 else 2
        ptrs, pitches, flags = self._source_planes(desc, planes, np.dtype(np.uint8 if es == 1 else np.uint16), es, None, asynchronous, who)
        if pitches[1] != pitches[2]:
            raise ValueError("the two chroma planes must share one pitch")
        pts = self._pts if pts is None else pts
        self._pts = pts + step
        entry = "send_frame_" + who[len("send_"):]
        args = ((C.byref(desc),) if by_ref else ()) + (ptrs[0], ptrs[1], ptrs[2], pitches[0], pitches[1], pts, flags)
        self._check(getattr(self._lib, "mihevc_" + entry)(self._s, *args), entry)

    def _send_rgb_planes(self, who, entry, fmt, width, height, size, planes, pts, asynchronous):
        """What send_rgb and send_sr share.  width, height: of the planes; size: the (width, height) arguments of the entries that take a source of its own
        size, () for the one that takes the session's."""
        shapes = fmt.plane_shapes(width, height)
        planes = list(planes)
        if fmt.layout and len(planes) == 1 and planes[0] is not None and tuple(planes[0].shape) == (height, width, fmt.layout):
            if isinstance(planes[0], np.ndarray) or planes[0].is_contiguous():
                planes[0] = planes[0].reshape(height, width * fmt.layout)
        if len(planes) != len(shapes) or any(p is None or tuple(p.shape) != s for p, s in zip(planes, shapes)):
            raise ValueError(f"plane shapes {[None if p is None else tuple(p.shape) for p in planes]} do not match {shapes} of {fmt!r} at {width}x{height}")
        es = fmt.element_size
        dt = np.dtype({1: np.float16, 2: np.float32}[fmt.sample]) if fmt.sample else np.dtype(np.uint8 if es == 1 else np.uint16)
        ptrs, pitches, flags = self._source_planes(fmt, planes, dt, es, bool(fmt.sample), asynchronous, who)
        if len(set(pitches)) != 1:
            raise ValueError("the three planes must share one pitch")
        pts = self._pts if pts is None else pts
        self._pts = pts + 1
        ptrs += [None] * (3 - len(ptrs))
        self._check(getattr(self._lib, "mihevc_" + entry)(self._s, C.byref(fmt), *size, ptrs[0], ptrs[1], ptrs[2], pitches[0], pts, flags), entry)

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
        self._send_planar("send_scaled", src, repr(src), src.width, src.height, src.bit_depth, [y, u, v], pts, 1, asynchronous)

    def send_deint(self, y, u, v, tff: bool = True, field_rate: bool = False, asynchronous: bool = False, pts: Optional[int] = None):
        """mihevc_send_frame_deint: a woven interlaced frame of the session's display size, planar 4:2:0 at the session's depth, deinterlaced on the device
        (DESIGN.md §6f).  tff: the top field (even rows) is the first in time.  field_rate: two pictures per frame, pts and pts + 1: the session is opened at
        twice the frame rate and pts counts field periods (the default pts advances by 2).  The frame's picture(s) come out once the next frame has arrived,
        the last frame's with flush().  Width even, height a multiple of 4, both at least 16; field order and rate are those of the first call.  numpy planes
        are checked for shape and type here; torch tensors on the device are read where they are (MIHEVC_SRC_DEVICE) under the rules of send_fmt.
        asynchronous (host planes): the rules of send_async."""
        c = self.cfg
        mode = _lib.Deint(int(bool(tff)), int(bool(field_rate)))
        self._send_planar("send_deint", mode, "the session", c.width, c.height, c.bit_depth, [y, u, v], pts, 2 if field_rate else 1, asynchronous)

    def send_fieldmatch(self, y, u, v, tff: bool = True, decimate: bool = True, deint: bool = True, asynchronous: bool = False, pts: Optional[int] = None):
        """mihevc_send_frame_fieldmatch: a woven frame of the session's display size, planar 4:2:0 at the session's depth, that carries film in fields (3:2
        pulldown): inverse telecine on the device.  tff: the declared field order.  decimate: of every five frames the repeat is dropped and the
        pictures are numbered pts_first, pts_first + 1, ...: the session is opened at 4/5 of the source rate.  deint: frames that stay combed are deinterlaced.
        A frame is decided once the next one has arrived, the last one with flush(); with decimate its picture waits for the cycle's fifth frame.  Every call
        waits for the metrics of the frame before, so an asynchronous one returns with less in flight than send_async does.  Geometry, planes and the mode of
        the first call: the rules of send_deint; no other send_* may follow before flush()."""
        c = self.cfg
        mode = _lib.Fieldmatch(int(bool(tff)), int(bool(decimate)), int(bool(deint)))
        self._send_planar("send_fieldmatch", mode, "the session", c.width, c.height, c.bit_depth, [y, u, v], pts, 1, asynchronous)

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
        self._send_planar("send_denoise", dn, "the session", c.width, c.height, c.bit_depth, [y, u, v], pts, 1, asynchronous)

    def send_interpolate(self, y, u, v, factor: int = 2, mode: str = 'mc', scene_threshold: int = 10, asynchronous: bool = False, pts: Optional[int] = None):
        """mihevc_send_frame_interpolate: a progressive frame of the session's display size, planar 4:2:0 at the session's depth; between it and the next frame
        factor - 1 pictures are interpolated on the device.  factor: 2, 3 or 4 pictures per frame; mode: 'mc' (motion compensated) or 'blend';
        both are those of the session's first call.  scene_threshold: 0 .. 255 in 8-bit units of mean absolute luma difference, 0 for no scene check; a pair of
        frames above it repeats its nearer frame.  Frame k's pictures come out at pts, pts + 1, .. once the next frame has arrived, the last frame's own picture
        with flush(): the caller numbers pts `factor` apart (the default does) and opens the session at factor times the source rate.  Width and height even and
        at least 16.  Planes and asynchronous: the rules of send_denoise."""
        c = self.cfg
        m = _lib.interpolate_mode(factor, mode, scene_threshold)
        self._send_planar("send_interpolate", m, "the session", c.width, c.height, c.bit_depth, [y, u, v], pts, m.factor, asynchronous)

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
        self._send_planar("send_chain", c, repr(c), c.width, c.height, c.bit_depth, [y, u, v], pts, 1, asynchronous, by_ref=False)

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
        self._send_planar("send_lut3d", src, "the session", c.width, c.height, src.bit_depth, [y, u, v], pts, 1, asynchronous)

    def send_upscaled(self, width: int, height: int, y, u, v, bit_depth: Optional[int] = None, sharpen: int = 8, antiring: int = 8, pts: Optional[int] = None,
                      asynchronous: bool = False):
        """mihevc_send_frame_upscaled: a planar 4:2:0 picture of width x height samples (per axis between a quarter of the session's size and that size), enlarged
        to the session's size on the device: Catmull-Rom interpolation, blended `antiring` eighths (0 .. 8) into the range of the two nearest
        samples, then on luma a limited 3x3 sharpener of gain `sharpen` sixteenths (0 .. 64, 0: off); both may change from picture to picture.  bit_depth,
        the planes and asynchronous: as send_scaled."""
        src = _lib.UpscaleSrc(int(width), int(height), int(self.cfg.bit_depth if bit_depth is None else bit_depth), int(sharpen), int(antiring))
        self._send_planar("send_upscaled", src, repr(src), src.width, src.height, src.bit_depth, [y, u, v], pts, 1, asynchronous)

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
        self._send_rgb_planes("send_sr", _entry, fmt, int(width), int(height), (int(width), int(height)), planes, pts, asynchronous)

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
        self._send_planar("send_sr_yuv", src, repr(src), src.width, src.height, src.bit_depth, [y, u, v], pts, 1, asynchronous)

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
        self._send_rgb_planes("send_rgb", "send_frame_rgb", fmt, self.cfg.width, self.cfg.height, (), planes, pts, asynchronous)

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


# the file-level code: hevc_amd.file_encode looks the sessions and config_for up in this module when it calls them, so it is imported last
from .file_encode import CHAIN_KEYS, encode_file, remux_audio, sr_target_size, upscale_target      # noqa: E402,F401
