"""What the tests of frame-rate multiplication (test_mcfi_cpu, test_gpu_mcfi and its child process mcfi_device_child) share: the display sizes and content kinds,
their inputs and model outputs, computed once, and the small sessions of the GPU tests."""
import ctypes as C
import functools

import numpy as np

from tests import mcfi_ref as R
from tests.ingest_common import base_cfg

# display sizes against the search tile of 8 x 8 blocks (64 x 64 luma samples) and the render tile of 64 x 32 samples of a plane: 16x16 (every window clamps on all
# sides); 70x36 (partial blocks right and bottom; chroma 35x18 ends in the middle of a chroma block); 72x72 (one block more than a search tile and more than a luma
# render tile in each direction); 138x74 (chroma 69x37: more than a chroma render tile in each direction, and the chroma tiles end in the middle of a block)
SIZES = [(16, 16), (70, 36), (72, 72), (138, 74)]
PANS = {"pan8": (8, -4), "pan36": (36, 36), "pan-36": (-36, 12), "pan48": (48, 0)}          # d = (dx, dy) from C to N; the last is out of range
KINDS = ("flat", "noise", "object", "cut") + tuple(PANS)
FACTORS = (2, 3, 4)


def texture(h, w, seed, lo=16, hi=235):
    """a smooth texture, 8-bit values: uniform noise under two 5 x 5 box filters, stretched to lo .. hi"""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 256, (h + 16, w + 16)).astype(np.int64)
    for _ in range(2):
        c = np.cumsum(np.cumsum(np.pad(t, ((1, 0), (1, 0))), axis=0), axis=1)
        t = c[5:, 5:] - c[:-5, 5:] - c[5:, :-5] + c[:-5, :-5]
    t = t[:h, :w]
    t0, t1 = int(t.min()), int(t.max())
    return lo + (t - t0) * (hi - lo) // max(t1 - t0, 1)


def wavy(h, w, seed, fine=32):
    """six long waves (70 .. 160 samples, any direction) under the detail of texture(): the half-size search sees the waves, the full-size one the detail"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    t = np.zeros((h, w))
    for _ in range(6):
        per, ang, ph = rng.uniform(70, 160), rng.uniform(0, np.pi), rng.uniform(0, 2 * np.pi)
        t += np.sin(2 * np.pi * (x * np.cos(ang) + y * np.sin(ang)) / per + ph)
    t = 128 + t * (80 / np.abs(t).max())
    return np.clip(np.rint(t).astype(np.int64) + texture(h, w, seed + 1, 0, fine) - fine // 2, 0, 255)


def planes_of(luma8, depth, seed):
    """a frame (Y, Cb, Cr) at `depth` from 8-bit luma: chroma is the 2x2-decimated luma, mirrored in value for Cr"""
    y = luma8 << (depth - 8)
    u = y[0::2, 0::2]
    v = ((1 << depth) - 1) - u
    return tuple(np.ascontiguousarray(p).astype(R.dtype(depth)) for p in (y, u, v))


def pan_frames(size, depth, d, seed=5, n=2, lo=16, hi=235):
    """n frames of a texture that moves by d = (dx, dy) per frame: frame k [y, x] = T[y - k dy, x - k dx]"""
    w, h = size
    dx, dy = d
    m = (n - 1) * max(abs(dx), abs(dy))
    T = texture(h + 2 * m, w + 2 * m, seed, lo, hi)
    return [planes_of(T[m - k * dy:m - k * dy + h, m - k * dx:m - k * dx + w], depth, seed) for k in range(n)]


@functools.lru_cache(maxsize=None)
def frames(size, depth, kind):
    """(C, N), each (Y, Cb, Cr).  At 10 bit the `noise` kind carries garbage above bit 9 in every other sample or so"""
    w, h = size
    rng = np.random.default_rng(w * 131 + h * 7 + depth + len(kind))
    if kind == "flat":
        f = planes_of(np.full((h, w), 77, np.int64), depth, 0)
        return f, f
    if kind == "noise":
        def plane(s):
            p = rng.integers(0, 1 << depth, s)
            return (p | (rng.integers(0, 64, s) * rng.integers(0, 2, s) << 10) if depth > 8 else p).astype(R.dtype(depth))
        return tuple(tuple(plane(s) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2))) for _ in range(2))
    if kind == "cut":
        return planes_of(texture(h, w, 1), depth, 0), planes_of(255 - texture(h, w, 2), depth, 0)
    if kind == "object":          # a textured square that moves by (6, 2) over a static texture
        bg, ob = texture(h, w, 3), texture(h, w, 4)
        out = []
        for k in range(2):
            t = bg.copy()
            x0, y0, s = w // 4 + 6 * k, h // 4 + 2 * k, min(w, h) // 3
            t[y0:y0 + s, x0:x0 + s] = ob[:s, :s]
            out.append(planes_of(t, depth, 0))
        return tuple(out)
    return tuple(pan_frames(size, depth, PANS[kind]))


@functools.lru_cache(maxsize=None)
def model_vectors(size, depth, kind):
    c, n = frames(size, depth, kind)
    return R.vectors(c[0], n[0], depth)


@functools.lru_cache(maxsize=None)
def model_picture(size, depth, kind, f, j, mode=0, scene_threshold=10):
    c, n = frames(size, depth, kind)
    _, v, D = model_vectors(size, depth, kind) if mode == 0 else (None, None, 0)
    return R.render(c, n, depth, f, j, v, D, mode, scene_threshold)


def extreme_fields(size):
    """fields no search gives: +-18 in every block, and signs alternating from block to block"""
    w, h = size
    nby, nbx = R.blocks(h), R.blocks(w)
    out = []
    for sx, sy in ((1, 1), (-1, -1), (1, -1), (-1, 1)):
        out.append(np.broadcast_to(np.array([sx * R.VMAX, sy * R.VMAX], np.int16), (nby, nbx, 2)).copy())
    alt = np.where((np.add.outer(np.arange(nby), np.arange(nbx)) & 1)[..., None] == 1, R.VMAX, -R.VMAX).astype(np.int16)
    out.append(np.concatenate([alt, -alt], axis=2).copy())
    return out


def plane_pointers(frame):
    return (C.c_void_p * 3)(*[p.ctypes.data for p in frame])


def interpolate_struct(f, mode=0, scene_threshold=10):
    from hevc_amd import _lib
    return _lib.Interpolate(f, mode, scene_threshold)


# ------------------------------------------------------------------------------------------------ GPU sessions
W, H, N_FRAMES = 100, 68, 5           # coded 104x72: a margin on both axes


def cfg_of(depth):
    cfg = base_cfg(depth)
    cfg.width, cfg.height = W, H
    return cfg


@functools.lru_cache(maxsize=None)
def clip(depth, n=N_FRAMES):
    """a gentle texture that pans by (6, -2) per frame, with a cut to a darker one that pans by (-4, 4) before the last but one frame"""
    a = pan_frames((W, H), depth, (6, -2), seed=21, n=n, lo=108, hi=148)
    b = pan_frames((W, H), depth, (-4, 4), seed=22, n=n, lo=30, hi=70)
    return tuple(a[k] if k < n - 2 else b[k] for k in range(n))


@functools.lru_cache(maxsize=None)
def model_pictures(depth, f, mode=0, n=N_FRAMES):
    """[(pts, display-size planes)] of the clip under the session's sequence rules: frame k has pts f k"""
    pics = R.clip_pictures(list(clip(depth, n)), depth, f, mode)
    return [(i, [p[:H, :W] if c == 0 else p[:H // 2, :W // 2] for c, p in enumerate(planes)]) for i, planes in enumerate(pics)]
