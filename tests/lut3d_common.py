"""What the tests of the colour table source (test_lut3d_cpu, test_gpu_lut3d and its child process lut3d_device_child) share: the display sizes, the cases the
stepped kernel and the device kernel are compared on, their inputs, tables and model outputs, computed once, and the small sessions of the GPU tests."""
import ctypes as C
import functools
from collections import namedtuple

import numpy as np

from tests import lut3d_ref as R
from tests.ingest_common import base_cfg

# display sizes against the kernel's tile of 256 x 32 source pixels and a lane's block of 16 x 2: 16x16 (the smallest: one block across); 70x36 (a margin on both
# axes: coded 72x40, the last block of a row half a block, a second tile of four rows down); 520x72 (two full tiles and a partial one on each axis) and 136x20
# (fewer rows than a tile)
SIZES = [(16, 16), (70, 36), (520, 72), (136, 20)]
NS = (2, 17, 33, 65)
KINDS = ("noise", "ramp", "cells")
MATRICES = (1, 5, 6, 9)

# B, D: source and output depth; n: points per axis; matrix / full: of the source; out_matrix / out_full: of the output
Case = namedtuple("Case", "size B D n kind matrix full out_matrix out_full")


def _cases():
    out, k = [], 0
    for size in SIZES:
        for B in (8, 10, 12):
            for D in (8, 10):
                for kind in KINDS:
                    out.append(Case(size, B, D, NS[k % 4], kind, MATRICES[(k // 4 + k) % 4], (k // 2) % 2, MATRICES[(k // 3 + 2 * k) % 4], (k // 5) % 2))
                    k += 1
    return out


CASES = _cases()


def case_id(c):
    return f"{c.size[0]}x{c.size[1]}-b{c.B}-d{c.D}-n{c.n}-{c.kind}-m{c.matrix}{'f' if c.full else 'l'}-m{c.out_matrix}{'f' if c.out_full else 'l'}"


@functools.lru_cache(maxsize=None)
def table(n):
    """a random table of n points per axis with the entries 0 and 65535 among them"""
    return R.random_table(n, 7 * n + 1)


@functools.lru_cache(maxsize=None)
def source(size, B, kind, n):
    return tuple(R.source(kind, size[0], size[1], B, seed=3, n=n))


@functools.lru_cache(maxsize=None)
def model(case):
    """planes of the coded size"""
    c = case
    return tuple(R.convert(source(c.size, c.B, c.kind, c.n), c.B, c.matrix, c.full, table(c.n), c.D, c.out_matrix, c.out_full))


def src_struct(B, matrix, full):
    from hevc_amd import _lib
    return _lib.Lut3dSrc(B, matrix, 1 if full else 0)


def vp(a):
    return C.c_void_p(a.ctypes.data)


# ------------------------------------------------------------------------------------------------ GPU sessions
W, H, N_FRAMES = 100, 68, 7           # coded 104x72: a margin on both axes
SRC_B, SRC_MATRIX = 10, 9             # the clip: 10 bit, BT.2020, limited range


def cfg_of(depth):
    cfg = base_cfg(depth)
    cfg.width, cfg.height = W, H
    cfg.matrix = 1
    return cfg


@functools.lru_cache(maxsize=None)
def clip(n=N_FRAMES):
    """a moving 10-bit picture: a diagonal luma gradient with a bright square that moves four samples a frame, chroma gradients, a little noise"""
    rng = np.random.default_rng(21)
    ys, xs = np.mgrid[0:H, 0:W]
    out = []
    for i in range(n):
        y = 64 + ((xs * 5 + ys * 7 + 11 * i) % 800)
        y[20:44, 10 + 4 * i:34 + 4 * i] = 900
        y = y + rng.integers(-3, 4, y.shape)
        u = 512 + ((xs[::2, ::2] * 3 + 5 * i) % 300) - 150
        v = 512 + ((ys[::2, ::2] * 4 + 3 * i) % 300) - 150
        out.append(tuple(np.ascontiguousarray(p.clip(0, 1023).astype("<u2")) for p in (y, u, v)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def session_table(which):
    """two different tables of two different sizes"""
    return R.random_table(33, 5) if which == 0 else R.random_table(17, 9)


@functools.lru_cache(maxsize=None)
def model_pictures(depth, tables):
    """display-size planes of every frame of the clip at the session's depth; tables: per frame, which session_table it is sent under (None: the frame is sent as
    it is, its 10-bit samples cut to the session's depth by dropping the low bits)"""
    out = []
    for planes, which in zip(clip(), tables):
        if which is None:
            out.append([np.ascontiguousarray((p >> (10 - depth)).astype(R.dtype(depth))) for p in planes])
        else:
            full = R.convert(planes, SRC_B, SRC_MATRIX, 0, session_table(which), depth, 1, 0)
            out.append([np.ascontiguousarray(p[:H, :W] if i == 0 else p[:H // 2, :W // 2]) for i, p in enumerate(full)])
    return out
