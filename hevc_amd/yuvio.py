"""Raw clip IO and the deterministic synthetic clips of the measurement plan.

The reference generates its test inputs with `ffmpeg -f lavfi -i testsrc=...` (tests/generate_test_videos.py:26-31)
and decodes arbitrary containers inside ffmpeg (core/transcoder.py:461).  Neither is possible without ffmpeg, so
the native path reads planar 4:2:0 / 4:2:2 / 4:4:4 at 8 .. 16 bit directly (`.y4m`, or `.yuv` named
`<stem>_<W>x<H>_<fps>[_422|_444][_<N>bit][_hdr].yuv`) and, when ffmpeg IS present, any other container through an `ffmpeg -f rawvideo` pipe.
A clip that is not planar 4:2:0 at the session's depth carries its layout in `src_format` and yields planes in its own shapes: the session
converts them on the device (Encoder.send_fmt).
"""
from __future__ import annotations

import re
import shutil
import subprocess
import tempfile
from fractions import Fraction
from pathlib import Path
from typing import Iterator, Optional, Tuple

import numpy as np

Planes = Tuple[np.ndarray, np.ndarray, np.ndarray]
_YUV_NAME = re.compile(r'_(\d+)x(\d+)_(\d+(?:\.\d+)?)(?:fps)?(?:_(420|422|444))?(?:_(8|9|10|12|14|16)bit)?(?:_(hdr|sdr))?$', re.I)
_Y4M_COLOUR = re.compile(r'C(420|422|444)(?:p(9|10|12|14|16)|jpeg|mpeg2|paldv)?$')


def _planar_format(chroma: int, depth: int):
    """(session bit depth, src_format): src_format is None for the plain layout, planar 4:2:0 at 8 or 10 bit"""
    from ._lib import SrcFormat
    return (10 if depth > 8 else 8), (None if chroma == 420 and depth in (8, 10) else SrcFormat(chroma, 0, depth, 0))


def _split_frame(a: np.ndarray, w: int, h: int, fmt) -> Planes:
    """one frame's elements -> planes: 4:2:0 without a format, else the format's own shapes (semi-planar: u is the interleaved plane, v is None)"""
    if fmt is None:
        return a[:w * h].reshape(h, w), a[w * h:w * h * 5 // 4].reshape(h // 2, w // 2), a[w * h * 5 // 4:].reshape(h // 2, w // 2)
    rows, row = fmt.chroma_shape(w, h)
    y, c = a[:w * h].reshape(h, w), a[w * h:]
    if fmt.semi_planar:
        return y, c.reshape(rows, row), None
    return y, c[:rows * row].reshape(rows, row), c[rows * row:].reshape(rows, row)


class Clip:
    """A planar clip on disk.  bit_depth: of the session that codes it (8, or 10 for anything deeper than 8); src_format: an _lib.SrcFormat when the
    frames are not planar 4:2:0 at that depth (frames() then yields planes in the source's own shapes), else None."""

    def __init__(self, path: Path, width: int, height: int, fps: float, bit_depth: int, n_frames: int, data_offset: int,
                 frame_header: int = 0, hdr: bool = False, src_format=None, interlace: str = 'p'):
        self.interlace = interlace      # the y4m interlace tag: 'p' progressive, 't' top field first, 'b' bottom field first ('m' mixed); raw .yuv: 'p'
        self.path, self.width, self.height, self.fps, self.bit_depth = Path(path), width, height, fps, bit_depth
        self.n_frames, self.data_offset, self.frame_header, self.hdr = n_frames, data_offset, frame_header, hdr
        self.src_format = src_format
        self._f = open(self.path, 'rb')

    @property
    def frame_bytes(self) -> int:
        if self.src_format is not None:
            return self.src_format.frame_bytes(self.width, self.height)
        return self.width * self.height * 3 // 2 * (2 if self.bit_depth > 8 else 1)

    def frames(self) -> Iterator[Planes]:
        dt = np.dtype('<u2') if self.bit_depth > 8 else np.uint8
        w, h = self.width, self.height
        self._f.seek(self.data_offset)
        for _ in range(self.n_frames):
            if self.frame_header:
                line = self._f.readline()
                if not line.startswith(b'FRAME'):
                    return
            buf = self._f.read(self.frame_bytes)
            if len(buf) < self.frame_bytes:
                return
            yield _split_frame(np.frombuffer(buf, dt), w, h, self.src_format)

    def close(self):
        self._f.close()


def open_clip(path: Path) -> Clip:
    path = Path(path)
    if path.suffix.lower() == '.y4m':
        with open(path, 'rb') as f:
            header = f.readline()
        if not header.startswith(b'YUV4MPEG2'):
            raise ValueError('not a YUV4MPEG2 file')
        w = h = 0
        fps, depth, chroma, interlace = 30.0, 8, 420, 'p'
        for tok in header.split()[1:]:
            t = tok.decode()
            if t[0] == 'W':
                w = int(t[1:])
            elif t[0] == 'H':
                h = int(t[1:])
            elif t[0] == 'F':
                n, d = t[1:].split(':')
                fps = int(n) / int(d) if int(d) else 30.0
            elif t[0] == 'I' and len(t) == 2:
                interlace = t[1]
            elif t[0] == 'C':
                m = _Y4M_COLOUR.match(t)
                if not m:
                    raise ValueError(f'unsupported chroma format {t}')
                chroma, depth = int(m.group(1)), int(m.group(2) or 8)
        depth, fmt = _planar_format(chroma, depth)
        fb = fmt.frame_bytes(w, h) if fmt is not None else w * h * 3 // 2 * (2 if depth > 8 else 1)
        n_frames = (path.stat().st_size - len(header)) // (fb + 6)
        return Clip(path, w, h, fps, depth, n_frames, len(header), frame_header=6, hdr=depth > 8 and 'hdr' in path.stem.lower(), src_format=fmt,
                    interlace=interlace)
    m = _YUV_NAME.search(path.stem)
    if not m:
        raise ValueError('raw .yuv needs <stem>_<W>x<H>_<fps>[_422|_444][_<N>bit][_hdr].yuv')
    w, h, fps = int(m.group(1)), int(m.group(2)), float(m.group(3))
    depth, fmt = _planar_format(int(m.group(4) or 420), int(m.group(5) or 8))
    fb = fmt.frame_bytes(w, h) if fmt is not None else w * h * 3 // 2 * (2 if depth > 8 else 1)
    return Clip(path, w, h, fps, depth, path.stat().st_size // fb, 0, hdr=(m.group(6) or '').lower() == 'hdr', src_format=fmt)


class _PipeClip:
    """Any container decoded by an `ffmpeg -f rawvideo` child (only when ffmpeg exists on this host).  A decode error or a short
    stream raises: a truncated clip must not come out as SUCCESS.  A probed sample format the device conversion covers (_lib.src_format_for) is
    asked for as it is, so swscale has nothing to do, and comes out with `src_format` set; anything else is asked for as planar 4:2:0, and so
    are the full-range yuvj* formats: there is no range conversion on the device, swscale's stays in front of them.  rgb_formats (opt-in): a probed
    RGB format of _lib.rgb_format_for is asked for as it is too, and the clip carries `rgb_format`: frames() then yields the three planes in the
    format's own order, or the one packed (height, layout * width) plane, for Encoder.send_rgb; a source deeper than 8 bit makes a 10-bit session."""

    def __init__(self, path: Path, info, native_formats: bool = True, rgb_formats: bool = False):
        self.width, self.height, self.fps = info.width, info.height, info.fps
        from .encoder import bit_depth_of
        self.bit_depth = bit_depth_of(info)
        self.n_frames = info.nb_frames or (int(info.duration * info.fps) if info.duration and info.fps else 0)
        pix = 'yuv420p10le' if self.bit_depth > 8 else 'yuv420p'
        from ._lib import SrcFormat, src_format_for
        name = (info.pix_fmt or '').lower()
        fmt = None if name.startswith('yuvj') or not native_formats else src_format_for(name)
        self.src_format = None
        if fmt is not None:
            pix = name
            if fmt != SrcFormat(420, 0, self.bit_depth, 0):
                self.src_format = fmt
        self.rgb_format = None
        if rgb_formats and native_formats and fmt is None:
            from ._lib import rgb_format_for
            self.rgb_format = rgb_format_for(name)
            if self.rgb_format is not None:
                pix = name
                self.bit_depth = 10 if self.bit_depth > 8 or self.rgb_format.element_size > 1 else 8
        self._name = Path(path).name
        # stderr goes to a file, not a pipe: a damaged input can make `-v error` write more than a pipe buffer holds before the first frame, and a
        # child blocked on stderr while frames() blocks on stdout would hang the encode for ever instead of failing it
        self._err = tempfile.TemporaryFile()
        self._p = subprocess.Popen(['ffmpeg', '-v', 'error', '-i', str(path), '-f', 'rawvideo', '-pix_fmt', pix, '-'],
                                   stdout=subprocess.PIPE, stderr=self._err)

    def frames(self) -> Iterator[Planes]:
        w, h, fmt, rgb = self.width, self.height, self.src_format, self.rgb_format
        fb = fmt.frame_bytes(w, h) if fmt is not None else w * h * 3 // 2 * (2 if self.bit_depth > 8 else 1)
        dt = np.dtype('<u2') if (fmt.bit_depth if fmt is not None else self.bit_depth) > 8 else np.uint8
        if rgb is not None:
            fb = rgb.frame_bytes(w, h)
            dt = np.dtype('<f4') if rgb.sample == 2 else np.dtype('<f2') if rgb.sample == 1 else np.dtype('<u2') if rgb.element_size == 2 else np.uint8
        n = 0
        while True:
            buf = self._p.stdout.read(fb)
            if len(buf) < fb:
                break
            n += 1
            if rgb is not None:
                yield tuple(np.frombuffer(buf, dt).reshape(len(rgb.plane_shapes(w, h)), *rgb.plane_shapes(w, h)[0]))
            else:
                yield _split_frame(np.frombuffer(buf, dt), w, h, fmt)
        rc = self._p.wait()
        self._err.seek(0, 2)
        self._err.seek(max(0, self._err.tell() - 2000))
        err = self._err.read().decode('utf-8', 'replace')[-500:]
        if rc != 0:
            raise RuntimeError(f'{self._name}: ffmpeg decode failed (exit {rc}): {err}')
        if self.n_frames and n < self.n_frames - max(2, self.n_frames // 100):      # container frame counts can be off by a frame or two
            raise RuntimeError(f'{self._name}: decoded {n} of {self.n_frames} frames')

    def close(self):
        try:
            self._p.kill()
            self._p.wait()
        except Exception:
            pass
        try:
            self._p.stdout.close()
            self._err.close()
        except Exception:
            pass


def open_any(path: Path, info=None, native_formats: bool = True, rgb_formats: bool = False):
    """native_formats=False: a container's frames are asked of ffmpeg as planar 4:2:0 whatever its own format (for a consumer without send_fmt).
    rgb_formats=True: a container probed as an RGB format of _lib.rgb_format_for is asked for as it is (for a consumer with send_rgb)"""
    path = Path(path)
    if path.suffix.lower() in ('.y4m', '.yuv'):
        return open_clip(path)
    if shutil.which('ffmpeg') is None:
        raise RuntimeError(f'{path.name}: only .y4m/.yuv can be read without ffmpeg on this host')
    return _PipeClip(path, info, native_formats, rgb_formats)


def write_y4m(path: Path, frames, width: int, height: int, fps=30, bit_depth: int = 8, chroma: int = 420, src_depth: Optional[int] = None,
              interlace: str = 'p'):
    """chroma: 420 / 422 / 444, the frames' planes in that shape; src_depth: the samples' own depth (9 .. 16) when it is not bit_depth's 8 or 10; interlace: the
    header's I tag, 'p' progressive, 't' / 'b' woven frames with the top / bottom field first"""
    if interlace not in ('p', 't', 'b'):
        raise ValueError(f'interlace tag {interlace!r}')
    fr = Fraction(str(fps)).limit_denominator(1001)
    depth = src_depth if src_depth else (10 if bit_depth > 8 else 8)
    tag = f'C{chroma}p{depth}' if depth > 8 else ('C420jpeg' if chroma == 420 else f'C{chroma}')
    with open(path, 'wb') as f:
        f.write(f'YUV4MPEG2 W{width} H{height} F{fr.numerator}:{fr.denominator} I{interlace} A1:1 {tag}\n'.encode())
        dt = np.dtype('<u2') if depth > 8 else np.uint8
        for y, u, v in frames:
            f.write(b'FRAME\n')
            for p in (y, u, v):
                f.write(np.ascontiguousarray(p, dtype=dt).tobytes())


def write_yuv(path: Path, frames, bit_depth: int = 8):
    dt = np.dtype('<u2') if bit_depth > 8 else np.uint8
    with open(path, 'wb') as f:
        for y, u, v in frames:
            for p in (y, u, v):
                f.write(np.ascontiguousarray(p, dtype=dt).tobytes())


# ---------------------------------------------------------------------------------------------
# synthetic clips: deterministic from (pattern, seed, W, H, n, bit_depth)
# ---------------------------------------------------------------------------------------------
class SyntheticClip:
    """`bars`: static colour bars + sweeping gradient + frame counter block (mirrors lavfi testsrc's intent).
    `motion`: band-limited Gaussian texture translating (+3,+1) px/frame, two rectangles on independent paths,
    i.i.d. grain (sigma 2 LSB at 8 bit, 8 LSB at 10 bit) re-seeded per frame — the headline workload.
    `stress`: what a translational search and a per-GOP rate plan do not like — the texture ZOOMS (scale 1 .. 1.5 and back), the whole picture FADES to
    dark and back, twelve small occluders move on their own paths, one hard cut (frame n/2: another texture) and a one-frame white flash (frame n/4):
    for the rate-control / scene-cut / conformance tests, not a benchmark.
    grain, still (`motion` only; the defaults change nothing): the grain's sigma is multiplied by `grain` (0: the grain-free picture the noisy one was made
    from); `still`: texture and rectangles stay where frame 0 has them, only the grain changes from frame to frame."""

    def __init__(self, pattern: str, seed: int, width: int, height: int, n_frames: int, bit_depth: int = 8, fps: float = 30.0, grain: float = 1.0, still: bool = False):
        assert pattern in ('bars', 'motion', 'stress')
        self.pattern, self.seed, self.width, self.height, self.n_frames, self.bit_depth, self.fps = pattern, seed, width, height, n_frames, bit_depth, fps
        self.hdr = bit_depth > 8
        self.grain, self.still = float(grain), bool(still)
        self._tex = None

    def _texture(self):
        if self._tex is None:
            rng = np.random.default_rng(self.seed)
            th, tw = self.height + 64, self.width + 64
            t = rng.standard_normal((th, tw)).astype(np.float32)
            for _ in range(3):                       # box blur x3 ~ Gaussian, with wrap-around so the field tiles
                for ax in (0, 1):
                    t = sum(np.roll(t, k, ax) for k in range(-3, 4)) / 7.0
            t = (t - t.mean()) / (t.std() + 1e-6)
            self._tex = np.tile(t, (2, 2))          # tiled twice so a wrapped window is one contiguous slice
        return self._tex

    def frame(self, i: int) -> Planes:
        w, h, bd = self.width, self.height, self.bit_depth
        lo, hi = (16, 235) if bd == 8 else (64, 940)
        sc = 1 << (bd - 8)
        if self.pattern == 'bars':
            xs = np.arange(w)
            bar = (xs * 8 // w)
            lum = np.array([235, 210, 170, 145, 106, 81, 41, 16], np.float32)[bar]
            y = np.tile(lum, (h, 1))
            y[h * 3 // 4:] = ((xs + 4 * i) % w) * (219.0 / w) + 16          # sweeping gradient
            cb = np.array([128, 16, 166, 54, 202, 90, 240, 128], np.float32)[bar[::2]]
            cr = np.array([128, 146, 16, 34, 222, 240, 110, 128], np.float32)[bar[::2]]
            u, v = np.tile(cb, (h // 2, 1)), np.tile(cr, (h // 2, 1))
            blk = 32
            bits = [(i >> k) & 1 for k in range(8)]                            # frame counter block
            for k, b in enumerate(bits):
                y[8:8 + blk, 8 + k * blk:8 + (k + 1) * blk] = 235 if b else 16
            y, u, v = y * sc, u * sc, v * sc
        elif self.pattern == 'stress':
            n = max(2, self.n_frames)
            t = self._texture()
            if i >= n // 2:
                t = t[::-1, ::-1]                                  # the scene after the cut
            th, tw = t.shape[0] // 2, t.shape[1] // 2
            zoom = 1.0 + 0.5 * abs(np.sin(np.pi * i / 40.0))
            ys = (np.arange(h, dtype=np.float32) - h / 2) / zoom + h / 2 + 0.5 * i
            xs = (np.arange(w, dtype=np.float32) - w / 2) / zoom + w / 2 + 1.5 * i
            win = t[np.mod(np.rint(ys).astype(np.int64), th)[:, None], np.mod(np.rint(xs).astype(np.int64), tw)[None, :]]
            fade = 0.35 + 0.65 * abs(np.cos(np.pi * i / 55.0))
            y = 126 + 44 * win
            g = np.random.default_rng((self.seed + 7) * 100003 + i)
            for k in range(12):                                    # occluders: position from a per-object linear path
                rw, rh = w // (12 + k), h // (9 + k % 5)
                x0 = (37 * k * k + (3 + k % 7 - 3) * 2 * i) % max(1, w - rw)
                y0 = (91 * k + (k % 5 - 2) * 3 * i) % max(1, h - rh)
                y[y0:y0 + rh, x0:x0 + rw] = 40 + 17 * k
            y = 16 + (y - 16) * fade + 1.5 * g.standard_normal((h, w), dtype=np.float32)
            u = 128 + 30 * win[::2, ::2] * fade + g.standard_normal((h // 2, w // 2), dtype=np.float32)
            v = 128 - 22 * win[::2, ::2] * fade + g.standard_normal((h // 2, w // 2), dtype=np.float32)
            if i == n // 4:
                y = y * 0 + 225
            y, u, v = y * sc, u * sc, v * sc
        else:
            t = self._texture()
            th, tw = t.shape[0] // 2, t.shape[1] // 2
            m = 0 if self.still else i          # the frame whose geometry this one has
            r0, c0 = (1 * m) % th, (3 * m) % tw
            win = t[r0:r0 + h, c0:c0 + w]
            y = 126 + 38 * win
            # two rectangles on independent paths
            for k, (rw, rh, vx, vy, lum) in enumerate(((w // 8, h // 6, 5, 2, 200), (w // 10, h // 5, -4, 3, 60))):
                x0 = (w // 4 * (k + 1) + vx * m) % max(1, w - rw)
                y0 = (h // 3 * (k + 1) + vy * m) % max(1, h - rh)
                y[y0:y0 + rh, x0:x0 + rw] = lum
            g = np.random.default_rng((self.seed + 1) * 100003 + i)
            gy, gc = np.float32(2.0 * self.grain), np.float32(self.grain)
            y = y + gy * g.standard_normal((h, w), dtype=np.float32)
            yy, xx = np.mgrid[0:h // 2, 0:w // 2]
            u = 128 + 24 * win[::2, ::2] + gc * g.standard_normal((h // 2, w // 2), dtype=np.float32)
            v = 128 - 24 * win[::2, ::2] + 10 * np.sin((xx + 3 * m / 2) / 40.0).astype(np.float32) + gc * g.standard_normal((h // 2, w // 2), dtype=np.float32)
            y, u, v = y * sc, u * sc, v * sc
        dt = np.uint16 if bd > 8 else np.uint8
        return (np.clip(np.rint(y), lo, hi).astype(dt), np.clip(np.rint(u), lo, hi + 5 * sc).astype(dt), np.clip(np.rint(v), lo, hi + 5 * sc).astype(dt))

    def frames(self) -> Iterator[Planes]:
        for i in range(self.n_frames):
            yield self.frame(i)

    def close(self):
        pass
