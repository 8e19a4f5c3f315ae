"""What the tests of the deinterlacing source (test_deint_cpu, test_gpu_deint and its child process deint_device_child) share: the display sizes and the
keep x second combinations, their inputs and model outputs, computed once, and the small sessions of the GPU tests."""
import ctypes as C
import functools

from tests import deint_ref as R
from tests.ingest_common import base_cfg

# display sizes: 70x36 (a margin on both axes, one tile), 136x72 (two luma tiles across, three down; chroma 68x36: a tile and a bit down, half a run at the
# right edge) and 264x20 (fewer rows than a tile, three tiles across)
SIZES = [(70, 36), (136, 72), (264, 20)]
COMBOS = [(keep, second) for keep in (0, 1) for second in (0, 1)]
KINDS = ("noise", "woven")


@functools.lru_cache(maxsize=None)
def frames(size, depth, kind):
    """(P, C, N): three frames of full-range noise (10 bit: values above the depth too), or three consecutive frames of a woven moving sinusoid"""
    w, h = size
    if kind == "noise":
        return tuple(R.noise_frames(w, h, depth, w * h + depth))
    return tuple(R.woven_frames(w, h, depth, 3, tff=True, seed=w + depth))


@functools.lru_cache(maxsize=None)
def model(size, depth, kind, keep, second):
    """(planes of the coded size, branch counts)"""
    return R.deinterlace(*frames(size, depth, kind), depth, keep, second)


def plane_pointers(frame):
    return (C.c_void_p * 3)(*[p.ctypes.data for p in frame])


# ------------------------------------------------------------------------------------------------ GPU sessions
W, H, N_FRAMES = 100, 68, 7           # coded 104x72: a margin on both axes


def cfg_of(depth, field_rate=False):
    cfg = base_cfg(depth)
    cfg.width, cfg.height = W, H
    if field_rate:
        cfg.fps_num *= 2
    return cfg


@functools.lru_cache(maxsize=None)
def clip(depth, tff, n=N_FRAMES):
    return tuple(R.woven_frames(W, H, depth, n, tff=tff, seed=11 + depth))


@functools.lru_cache(maxsize=None)
def model_pictures(depth, tff, field_rate, n=N_FRAMES):
    """[(pts, display-size planes)] of the clip under the session's sequence rules"""
    return [(pts, [p[:H, :W] if i == 0 else p[:H // 2, :W // 2] for i, p in enumerate(planes)]) for pts, planes in R.pictures(list(clip(depth, tff, n)), depth, tff, field_rate)]
