"""What the tests of the denoising source (test_denoise_cpu, test_gpu_denoise and its child process denoise_device_child) share: the display sizes and the
strengths, their inputs and model outputs, computed once, and the small sessions of the GPU tests."""
import ctypes as C
import functools

from tests import denoise_ref as R
from tests.ingest_common import base_cfg

# display sizes against the kernel's tile of 128 x 32: 16x16 (the smallest: chroma 8x8, one run); 70x36 (a margin on both axes; one tile across, a second one of
# four rows down); 264x72 (two full tiles and a partial one on each axis; chroma 132x36: a full tile and half a run more, a tile and four rows down) and 136x20
# (fewer rows than a tile)
SIZES = [(16, 16), (70, 36), (264, 72), (136, 20)]
# nothing; everything; luma spatial only and chroma temporal only; level 2
STRENGTHS = [(0, 0, 0, 0), (255, 255, 255, 255), (12, 0, 0, 16), 2]
KINDS = ("noise", "moving")


def strength_id(s):
    return f"level{s}" if isinstance(s, int) else "-".join(str(t) for t in s)


@functools.lru_cache(maxsize=None)
def frames(size, depth, kind):
    """(P, C, N): three frames of full-range noise (10 bit: values above the depth too), or three consecutive frames of the pattern of the quality test moving 3
    samples per frame under noise of sigma 2"""
    w, h = size
    if kind == "noise":
        return tuple(R.noise_frames(w, h, depth, 3 * w * h + depth))
    return tuple(R.noisy_frames(w, h, depth, 3, 3, seed=w + depth)[0])


@functools.lru_cache(maxsize=None)
def model(size, depth, kind, strength):
    """(planes of the coded size, one Counter of weight classes per plane)"""
    return R.denoise(*frames(size, depth, kind), depth, strength)


def plane_pointers(frame):
    return (C.c_void_p * 3)(*[p.ctypes.data for p in frame])


def denoise_struct(strength):
    from hevc_amd import _lib
    return _lib.Denoise(*R.strengths(strength))


# ------------------------------------------------------------------------------------------------ GPU sessions
W, H, N_FRAMES = 100, 68, 7           # coded 104x72: a margin on both axes
CHANGING = [2, 2, (12, 0, 0, 16), 0, 3, (255, 255, 255, 255), 1]      # one strength per frame of the clip


def cfg_of(depth):
    cfg = base_cfg(depth)
    cfg.width, cfg.height = W, H
    return cfg


@functools.lru_cache(maxsize=None)
def clip(depth, n=N_FRAMES):
    return tuple(R.noisy_frames(W, H, depth, n, 3, seed=11 + depth)[0])


@functools.lru_cache(maxsize=None)
def model_pictures(depth, strength, n=N_FRAMES):
    """[(pts, display-size planes)] of the clip under the session's sequence rules; strength: one for all frames, or "changing": CHANGING"""
    per = list(CHANGING[:n]) if strength == "changing" else strength
    return [(pts, [p[:H, :W] if i == 0 else p[:H // 2, :W // 2] for i, p in enumerate(planes)]) for pts, planes in R.pictures(list(clip(depth, n)), depth, per)]
