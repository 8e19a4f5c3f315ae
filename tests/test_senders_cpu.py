"""CPU (-m "not gpu"): what the source senders of hevc_amd.encoder.Encoder hand to the C entries.  A stand-in library records every mihevc_send_frame_* call, so
no device is needed: per sender the entry, the descriptor's fields, the three pointers, the pitches, the pts and the flags for host, asynchronous and device
planes, the session's pts counter afterwards, and the exact text of the ValueError for a wrong shape, a wrong sample type and a chroma pitch that differs."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from hevc_amd import _lib
from hevc_amd.encoder import Encoder

W, H = 32, 16             # the session
SW, SH = 64, 32           # a source of its own size
HANDLE = 0x5e55


class Recorder(SimpleNamespace):
    """stands where the loaded library would: every mihevc_send_frame_* keeps its name and arguments (a byref() argument: the struct's bytes) and returns 0"""

    def __init__(self):
        super().__init__(calls=[])

    def __getattr__(self, name):
        if not name.startswith("mihevc_send_frame_"):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append((name,) + tuple(bytes(a._obj) if hasattr(a, "_obj") else a.value if isinstance(a, C.c_void_p) else a for a in args))
            return 0
        return entry


class Tensor:
    """stands where a torch tensor on the device would: the interface Encoder._source_planes reads"""
    is_cuda = True

    def __init__(self, shape, es, ptr, pitch=None, floats=False):
        self.shape, self._es, self._ptr, self._pitch, self._floats = shape, es, ptr, pitch or shape[1] + 8, floats

    def element_size(self):
        return self._es

    def is_floating_point(self):
        return self._floats

    def stride(self, k):
        return (self._pitch, 1)[k]

    def data_ptr(self):
        return self._ptr


def session(depth, chain=None):
    enc = Encoder.__new__(Encoder)
    enc._lib, enc._s, enc._pts = Recorder(), C.c_void_p(HANDLE), 0
    enc.cfg = _lib.Config()
    enc.cfg.width, enc.cfg.height, enc.cfg.bit_depth = W, H, depth
    if chain is not None:
        enc._chain = chain
    return enc


def ints(desc):
    """a descriptor as C sees it: its int32 words"""
    return tuple(np.frombuffer(bytes(desc), np.int32).tolist())


def yuv(w, h, dt):
    return [np.zeros((h, w), dt), np.zeros((h // 2, w // 2), dt), np.zeros((h // 2, w // 2), dt)]


def yuv_tensors(w, h, es, chroma_pitches=None):
    cp = chroma_pitches or (w // 2 + 8, w // 2 + 8)
    return [Tensor((h, w), es, 0x1000, w + 16), Tensor((h // 2, w // 2), es, 0x2000, cp[0]), Tensor((h // 2, w // 2), es, 0x3000, cp[1])]


def the_chain(d):
    return _lib.chain(SW, SH, d, denoise=2, resize="scale")


# sender -> (the entry, the source's size: the session's or its own, the call, the descriptor's leading words at depth d (None: none goes to C), what the
# messages call the source, the step of the pts counter)
PLANAR = {
    "send_scaled": ("scaled", (SW, SH), lambda e, p, **k: e.send_scaled(SW, SH, *p, **k), lambda d: (SW, SH, d), lambda d: repr(_lib.ScaleSrc(SW, SH, d)), 1),
    "send_deint": ("deint", (W, H), lambda e, p, **k: e.send_deint(*p, tff=False, **k), lambda d: (0, 0), lambda d: "the session", 1),
    "send_deint/field": ("deint", (W, H), lambda e, p, **k: e.send_deint(*p, field_rate=True, **k), lambda d: (1, 1), lambda d: "the session", 2),
    "send_fieldmatch": ("fieldmatch", (W, H), lambda e, p, **k: e.send_fieldmatch(*p, decimate=False, **k), lambda d: (1, 0, 1), lambda d: "the session", 1),
    "send_denoise": ("denoise", (W, H), lambda e, p, **k: e.send_denoise(*p, strength=(1, 2, 3, 4), **k), lambda d: (1, 2, 3, 4), lambda d: "the session", 1),
    "send_denoise/level": ("denoise", (W, H), lambda e, p, **k: e.send_denoise(*p, **k), lambda d: _lib.DENOISE_LEVELS[2], lambda d: "the session", 1),
    "send_denoise/struct": ("denoise", (W, H), lambda e, p, **k: e.send_denoise(*p, strength=_lib.Denoise(9, 8, 7, 6), **k), lambda d: (9, 8, 7, 6),
                            lambda d: "the session", 1),
    "send_interpolate": ("interpolate", (W, H), lambda e, p, **k: e.send_interpolate(*p, factor=3, mode="blend", scene_threshold=7, **k), lambda d: (3, 1, 7),
                         lambda d: "the session", 3),
    "send_interpolate/default": ("interpolate", (W, H), lambda e, p, **k: e.send_interpolate(*p, **k), lambda d: (2, 0, 10), lambda d: "the session", 2),
    "send_chain": ("chain", (SW, SH), lambda e, p, **k: e.send_chain(*p, **k), None, lambda d: repr(the_chain(d)), 1),
    "send_lut3d": ("lut3d", (W, H), lambda e, p, **k: e.send_lut3d(*p, bit_depth=e.cfg.bit_depth, matrix=9, full_range=True, **k), lambda d: (d, 9, 1),
                   lambda d: "the session", 1),
    "send_upscaled": ("upscaled", (SW, SH), lambda e, p, **k: e.send_upscaled(SW, SH, *p, sharpen=5, antiring=3, **k), lambda d: (SW, SH, d, 5, 3),
                      lambda d: repr(_lib.UpscaleSrc(SW, SH, d, 5, 3)), 1),
    "send_upscaled/default": ("upscaled", (SW, SH), lambda e, p, **k: e.send_upscaled(SW, SH, *p, **k), lambda d: (SW, SH, d, 8, 8),
                              lambda d: repr(_lib.UpscaleSrc(SW, SH, d, 8, 8)), 1),
    "send_sr_yuv": ("sr_yuv", (SW, SH), lambda e, p, **k: e.send_sr_yuv(SW, SH, *p, bit_depth=e.cfg.bit_depth, matrix=1, **k), lambda d: (SW, SH, d, 1, 0),
                    lambda d: repr(_lib.SrYuv(SW, SH, d, 1, 0)), 1),
}
# what _source_planes calls the source in its own message: the descriptor
FMT = {"send_deint": lambda d: _lib.Deint(0, 0), "send_deint/field": lambda d: _lib.Deint(1, 1), "send_fieldmatch": lambda d: _lib.Fieldmatch(1, 0, 1),
       "send_denoise": lambda d: _lib.Denoise(1, 2, 3, 4), "send_denoise/level": lambda d: _lib.denoise_level(2), "send_denoise/struct": lambda d: _lib.Denoise(9, 8, 7, 6),
       "send_interpolate": lambda d: _lib.Interpolate(3, 1, 7), "send_interpolate/default": lambda d: _lib.Interpolate(2, 0, 10), "send_lut3d": lambda d: _lib.Lut3dSrc(d, 9, 1)}


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("name", sorted(PLANAR))
def test_planar_sender_hands_c_the_planes_as_they_are(name, depth):
    entry, (w, h), call, words, of, step = PLANAR[name]
    dt, es = (np.uint8, 1) if depth == 8 else (np.uint16, 2)
    enc = session(depth, the_chain(depth))
    p = yuv(w, h, dt)
    t = yuv_tensors(w, h, es)
    enc._pts = 5
    call(enc, p)                                        # host planes, the default pts
    assert enc._pts == 5 + step
    call(enc, p, pts=11, asynchronous=True)             # asynchronous, a pts of the caller's
    assert enc._pts == 11 + step
    call(enc, t, pts=40)                                # planes on the device
    assert enc._pts == 40 + step
    call(enc, t, asynchronous=True)
    assert enc._pts == 40 + 2 * step
    host = (p[0].ctypes.data, p[1].ctypes.data, p[2].ctypes.data, w, w // 2)
    dev = (0x1000, 0x2000, 0x3000, w + 16, w // 2 + 8)
    want = [host + (5, 0), host + (11, _lib.SRC_ASYNC), dev + (40, _lib.SRC_DEVICE), dev + (40 + step, _lib.SRC_DEVICE | _lib.SRC_ASYNC)]
    assert len(enc._lib.calls) == 4
    for got, tail in zip(enc._lib.calls, want):
        assert got[0] == "mihevc_send_frame_" + entry and got[1] == HANDLE
        if words is None:
            assert got[2:] == tail
        else:
            desc = tuple(np.frombuffer(got[2], np.int32).tolist())
            assert desc[:len(words(depth))] == tuple(words(depth)) and not any(desc[len(words(depth)):])
            assert got[3:] == tail


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("name", sorted(PLANAR))
def test_planar_sender_refusals_word_for_word(name, depth):
    entry, (w, h), call, words, of, step = PLANAR[name]
    dt, other, es = (np.uint8, np.uint16, 1) if depth == 8 else (np.uint16, np.uint8, 2)
    enc = session(depth, the_chain(depth))
    shapes = [(h, w), (h // 2, w // 2), (h // 2, w // 2)]
    bad = yuv(w, h, dt)
    bad[2] = np.zeros((h // 2, w // 2 + 1), dt)
    with pytest.raises(ValueError) as e:
        call(enc, bad)
    assert str(e.value) == f"plane shapes {[(h, w), (h // 2, w // 2), (h // 2, w // 2 + 1)]} do not match {shapes} of {of(depth)}"
    with pytest.raises(ValueError) as e:
        call(enc, [bad[0], None, bad[1]])
    assert str(e.value) == f"plane shapes {[(h, w), None, (h // 2, w // 2)]} do not match {shapes} of {of(depth)}"
    # the shapes are judged before the types
    with pytest.raises(ValueError, match="^plane shapes"):
        call(enc, [p.astype(other) for p in bad])
    fmt = FMT[name](depth) if name in FMT else of(depth)
    fmt = fmt if isinstance(fmt, str) else repr(fmt)
    with pytest.raises(ValueError) as e:
        call(enc, yuv(w, h, other))
    assert str(e.value) == f"{[np.dtype(other).name] * 3} planes handed over as {fmt}"
    with pytest.raises(ValueError) as e:
        call(enc, yuv(w, h, other), asynchronous=True)
    assert str(e.value) == f"an asynchronous {name.split('/')[0]} needs C-contiguous planes of the format's element type"
    with pytest.raises(ValueError) as e:
        call(enc, [yuv(w, h, dt)[0]] + yuv_tensors(w, h, es)[1:])
    assert str(e.value) == "device planes must be tensors on the GPU of the format's element size with unit column stride"
    # the types are judged before the pitches
    with pytest.raises(ValueError, match="^device planes must be"):
        call(enc, yuv_tensors(w, h, 3 - es, (w, w + 2)))
    with pytest.raises(ValueError) as e:
        call(enc, yuv_tensors(w, h, es, (w, w + 2)))
    assert str(e.value) == "the two chroma planes must share one pitch"
    assert enc._pts == 0 and not enc._lib.calls


def test_send_chain_needs_set_chain():
    enc = session(8)
    with pytest.raises(_lib.MihevcError) as e:
        enc.send_chain(*yuv(SW, SH, np.uint8))
    assert e.value.code == _lib.ESTATE and "send_chain without set_chain" in str(e.value) and not enc._lib.calls


# ------------------------------------------------------------------------------------------------ the R'G'B' pair
RGB = {
    "send_rgb": ("rgb", (W, H), lambda e, f, p, **k: e.send_rgb(f, *p, **k), ()),
    "send_sr": ("sr", (SW, SH), lambda e, f, p, **k: e.send_sr(f, SW, SH, *p, **k), (SW, SH)),
    "send_sr_fit": ("sr_fit", (SW, SH), lambda e, f, p, **k: e.send_sr_fit(f, SW, SH, *p, **k), (SW, SH)),
}
RGB_FORMATS = {"u8": (lambda: _lib.RgbFormat(0, 0, 1, 2, 0, 8), np.uint8, np.uint16), "u16": (lambda: _lib.RgbFormat(0, 2, 0, 1, 0, 16), np.uint16, np.int8),
               "f32": (lambda: _lib.RgbFormat(0, 0, 1, 2, 2, 0), np.float32, np.uint32), "packed": (lambda: _lib.RgbFormat(4, 0, 1, 2, 0, 8), np.uint8, np.uint16)}


@pytest.mark.parametrize("kind", sorted(RGB_FORMATS))
@pytest.mark.parametrize("name", sorted(RGB))
def test_rgb_sender_hands_c_the_planes_as_they_are(name, kind):
    entry, (w, h), call, size = RGB[name]
    make, dt, _ = RGB_FORMATS[kind]
    fmt = make()
    es = np.dtype(dt).itemsize
    enc = session(8)
    shape = (h, w) if fmt.layout == 0 else (h, w * fmt.layout)
    n = 3 if fmt.layout == 0 else 1
    p = [np.zeros(shape, dt) for _ in range(n)]
    t = [Tensor(shape, es, 0x1000 * (k + 1), shape[1] + 8, floats=bool(fmt.sample)) for k in range(n)]
    enc._pts = 5
    call(enc, fmt, p)
    assert enc._pts == 6
    call(enc, fmt, p, pts=11, asynchronous=True)
    assert enc._pts == 12
    call(enc, fmt, t, pts=40)
    call(enc, fmt, t, asynchronous=True)
    assert enc._pts == 42
    if fmt.layout:                                      # one packed plane may come as (height, width, layout)
        call(enc, fmt, [p[0].reshape(h, w, fmt.layout)], pts=50)
    host = tuple(x.ctypes.data for x in p) + (None,) * (3 - n) + (shape[1],)
    dev = tuple(0x1000 * (k + 1) for k in range(n)) + (None,) * (3 - n) + (shape[1] + 8,)
    want = [host + (5, 0), host + (11, _lib.SRC_ASYNC), dev + (40, _lib.SRC_DEVICE), dev + (41, _lib.SRC_DEVICE | _lib.SRC_ASYNC)] + ([host + (50, 0)] if fmt.layout else [])
    assert len(enc._lib.calls) == len(want)
    for got, tail in zip(enc._lib.calls, want):
        assert got[:3] == ("mihevc_send_frame_" + entry, HANDLE, bytes(fmt)) and got[3:] == size + tail


@pytest.mark.parametrize("kind", sorted(RGB_FORMATS))
@pytest.mark.parametrize("name", sorted(RGB))
def test_rgb_sender_refusals_word_for_word(name, kind):
    entry, (w, h), call, size = RGB[name]
    make, dt, other = RGB_FORMATS[kind]
    fmt = make()
    es = np.dtype(dt).itemsize
    enc = session(8)
    shape = (h, w) if fmt.layout == 0 else (h, w * fmt.layout)
    n = 3 if fmt.layout == 0 else 1
    bad = [np.zeros(shape, dt) for _ in range(n - 1)] + [np.zeros((h + 1, shape[1]), dt)]
    with pytest.raises(ValueError) as e:
        call(enc, fmt, bad)
    assert str(e.value) == f"plane shapes {[shape] * (n - 1) + [(h + 1, shape[1])]} do not match {[shape] * n} of {fmt!r} at {w}x{h}"
    with pytest.raises(ValueError) as e:
        call(enc, fmt, [np.zeros(shape, dt)] * (n + 1))
    assert str(e.value) == f"plane shapes {[shape] * (n + 1)} do not match {[shape] * n} of {fmt!r} at {w}x{h}"
    with pytest.raises(ValueError, match="^plane shapes"):
        call(enc, fmt, [p.astype(other) for p in bad])
    with pytest.raises(ValueError) as e:
        call(enc, fmt, [np.zeros(shape, other) for _ in range(n)])
    assert str(e.value) == f"{[np.dtype(other).name] * n} planes handed over as {fmt!r}"
    with pytest.raises(ValueError) as e:
        call(enc, fmt, [np.zeros(shape, other) for _ in range(n)], asynchronous=True)
    assert str(e.value) == f"an asynchronous {'send_rgb' if name == 'send_rgb' else 'send_sr'} needs C-contiguous planes of the format's element type"
    with pytest.raises(ValueError) as e:                # an integer tensor for a float format and the other way round
        call(enc, fmt, [Tensor(shape, es, 0x1000, floats=not fmt.sample) for _ in range(n)])
    assert str(e.value) == "device planes must be tensors on the GPU of the format's element type with unit column stride"
    if n == 3:
        with pytest.raises(ValueError) as e:
            call(enc, fmt, [Tensor(shape, es, 0x1000 * (k + 1), shape[1] + 8 * k, floats=bool(fmt.sample)) for k in range(3)])
        assert str(e.value) == "the three planes must share one pitch"
    assert enc._pts == 0 and not enc._lib.calls
