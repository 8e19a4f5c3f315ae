"""What the tests of the Y'CbCr input of the learned super-resolution share (test_sr_yuv_cpu, test_gpu_sr_yuv and its child process sr_yuv_device_child): the
cases and sources of the kernel tests with the model's answer, computed once, the ctypes call that is the same for the stepped library (emu_) and the device
(mihevc_k_), and the clips, configurations and by-hand chains of the session tests."""
import ctypes as C
import functools
import itertools

import numpy as np

from hevc_amd import _lib
from tests import sr_common as S
from tests import sr_yuv_ref as Y
from tests import util

# every (B, matrix, full range, scale)
CASES = list(itertools.product((8, 10, 12), (1, 5, 6, 9), (False, True), (4, 2)))
# 4x4: one partial workgroup; 18x14 and 34x16: 63 and 136 of a workgroup's 256 blocks of 2 x 2 (252 and 544 pixels); 66x34: 561 blocks, two workgroups and a part
SIZES = [(4, 4), (18, 14), (34, 16), (66, 34)]
KINDS = ("random", "grey", "edges")


def case_id(c):
    return f"{c[0]}bit-m{c[1]}-{'full' if c[2] else 'limited'}-x{c[3]}"


@functools.lru_cache(maxsize=None)
def source(kind, w, h, B):
    """(y, u, v) tight planes.  random: uniform samples, at 10 and 12 bit raw values above 2^B - 1 too; grey: flat mid-grey; edges: mid-range chroma whose first row and column lie
    near one end of the range and whose last row and column near the other, under a luma ramp"""
    dt = np.uint8 if B == 8 else np.dtype("<u2")
    peak = (1 << B) - 1
    rng = np.random.default_rng(w * 1000 + h * 10 + B)
    if kind == "random":
        top = 256 if B == 8 else 1 << 16
        planes = [rng.integers(0, top, s) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2))]
        planes[0][0, 0], planes[0][0, 1] = 0, peak
    elif kind == "grey":
        planes = [np.full(s, 1 << (B - 1)) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2))]
    else:
        y = (np.arange(h)[:, None] * 3 + np.arange(w)[None, :] * 5) * peak // (3 * h + 5 * w)
        planes = [y]
        for first, last in ((peak - peak // 8, peak // 8), (peak // 6, peak - peak // 6)):
            c = np.full((h // 2, w // 2), peak // 2)
            c[0, :], c[:, 0] = first, first
            c[-1, :], c[:, -1] = last, last
            planes.append(c)
    return tuple(np.ascontiguousarray(p.astype(dt)) for p in planes)


@functools.lru_cache(maxsize=None)
def want(kind, w, h, B, matrix, full, scale):
    return Y.input_tensor(source(kind, w, h, B), B, matrix, full, scale)


def laid_out(p, pitch, off_one):
    """a copy of plane `p` with rows `pitch` elements apart that starts at a 64-byte boundary, or one element behind one; the view keeps its buffer alive"""
    es = p.itemsize
    buf = np.zeros(pitch * p.shape[0] + 64 // es + 1, p.dtype)
    start = (-buf.ctypes.data % 64) // es + (1 if off_one else 0)
    v = np.lib.stride_tricks.as_strided(buf[start:], p.shape, (pitch * es, es))
    v[...] = p
    return v


def run_from_yuv(lib, prefix, planes, B, matrix, full, scale, device=None, pitch_extra=(0, 0), off_one=False, order=0):
    """the tensor k_sr_from_yuv writes, [th, tw, 32] uint16.  pitch_extra: elements added to the luma / chroma pitch"""
    h, w = planes[0].shape
    py, pc = w + pitch_extra[0], w // 2 + pitch_extra[1]
    held = [laid_out(p, py if i == 0 else pc, off_one) for i, p in enumerate(planes)]
    f = 2 if scale == 2 else 1
    out = np.full((h // f, w // f, 32), 0xA5A5, np.uint16)
    src = _lib.SrYuv(w, h, B, matrix, 1 if full else 0)
    ptrs = [v.ctypes.data for v in held]
    if prefix == "emu_":
        lib.emu_sr_from_yuv.argtypes = [C.POINTER(_lib.SrYuv), C.c_int] + [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int]
        rc = lib.emu_sr_from_yuv(C.byref(src), scale, *ptrs, py, pc, util.ptr(out), int(off_one), order)
    else:
        rc = lib.mihevc_k_sr_from_yuv(device, C.byref(src), scale, *ptrs, py, pc, util.ptr(out))
    assert rc == 0, rc
    return out


def check_case(lib, prefix, case, device=None):
    """every size, kind, a pitch that is no multiple of 16 elements and a plane one element off an aligned address, against the model"""
    B, matrix, full, scale = case
    n = CASES.index(case)
    for k, ((w, h), kind) in enumerate(itertools.product(SIZES, KINDS)):
        extra, off = [(0, 0), (3, 5), (1, 1)][(n + k) % 3], bool((n + k) % 2)
        got = run_from_yuv(lib, prefix, source(kind, w, h, B), B, matrix, full, scale, device, extra, off, order=(n + k) % 3)
        exp = want(kind, w, h, B, matrix, full, scale)
        assert np.array_equal(got, exp), (w, h, kind, extra, off, np.argwhere(got != exp)[:4])


# ------------------------------------------------------------------------------------------------ sessions
def session_cfg(depth, w=S.SESSION_W, h=S.SESSION_H, matrix=1):
    cfg = S.session_cfg(depth)
    cfg.width, cfg.height, cfg.matrix = w, h, matrix
    return cfg


@functools.lru_cache(maxsize=None)
def yuv_clip(sw, sh, depth, n=S.SESSION_N):
    """n pictures of a moving scene as planar 4:2:0 planes"""
    out = []
    for i in range(n):
        f = util.synth_frame(max(sh, 40), max(sw, 48), seed=11, shift=(3 * i, 2 * i), bit_depth=depth)
        dt = np.uint16 if depth > 8 else np.uint8
        out.append(tuple(np.ascontiguousarray(np.asarray(p)[:r, :c].astype(dt)) for p, (r, c) in zip((f.y, f.u, f.v), ((sh, sw), (sh // 2, sw // 2), (sh // 2, sw // 2)))))
    return out


def rgb16_planes(planes, B, matrix, full):
    """the model's R'G'B' at 16 bit as gbrp16le planes (G, B, R order) and their format"""
    r, g, b = (np.ascontiguousarray(p.astype(np.uint16)) for p in Y.rgb16(planes, B, matrix, full))
    return _lib.rgb_format_for("gbrp16le"), [g, b, r]


def drain(enc):
    enc.flush()
    return b"".join(d for d, _, _ in enc.packets())


def intermediate_planes(lib, half_planes, matrix, full):
    """what the resized route scales down: the planes mihevc_k_convert_rgb (10 bit) makes of the network's half planes [3, H, W], cut to the display size"""
    _, h, w = half_planes.shape
    fmt = _lib.RgbFormat(*S.HALF_PLANES[:6], matrix, 2 if full else 1)
    pw, ph = (w + 7) // 8 * 8, (h + 7) // 8 * 8
    out = [np.zeros(s, np.uint16) for s in ((ph, pw), (ph // 2, pw // 2), (ph // 2, pw // 2))]
    src = [np.ascontiguousarray(p) for p in half_planes]
    rc = lib.mihevc_k_convert_rgb(0, C.byref(fmt), *[p.ctypes.data for p in src], w, h, w, 10, *[p.ctypes.data for p in out])
    assert rc == 0, rc
    return [np.ascontiguousarray(out[0][:h, :w]), np.ascontiguousarray(out[1][:h // 2, :w // 2]), np.ascontiguousarray(out[2][:h // 2, :w // 2])]
