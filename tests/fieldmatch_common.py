"""What the tests of inverse telecine (test_fieldmatch_cpu, test_gpu_fieldmatch and its child process fieldmatch_device_child) share: the film frames, the
telecined, noisy and hybrid clips made of them with the record of which film frame every field came from, the sizes of the kernel tests with their inputs, and the
small sessions of the GPU tests."""
import functools

import numpy as np

from tests import deint_ref as D
from tests import fieldmatch_ref as R
from tests.ingest_common import base_cfg

# display sizes of the kernel tests.  The metrics tile is 128 x 32 luma samples: 70x36 (one tile across with a partial 16- and 32-block and a run that straddles
# W, a second tile row of four rows), 136x72 (two tiles across, the second eight columns wide; three down, the last of eight rows) and 264x20 (three tiles across,
# fewer rows than a tile).  The weave has the deinterlacer's tiles: the same three sizes meet their edges (tests/deint_common.py)
SIZES = [(70, 36), (136, 72), (264, 20)]
W, H = 136, 72           # the clips


# ------------------------------------------------------------------------------------------------ film
@functools.lru_cache(maxsize=None)
def _texture(seed, rows, cols, fy, fx):
    """band-limited noise in [0.08, 0.92]: nothing above fy cycles per sample down and fx across"""
    rng = np.random.default_rng(seed)
    spec = np.fft.fft2(rng.normal(size=(rows, cols)))
    ky, kx = np.abs(np.fft.fftfreq(rows))[:, None], np.abs(np.fft.fftfreq(cols))[None, :]
    spec[(ky > fy) | (kx > fx) | ((ky == 0) & (kx == 0))] = 0
    t = np.real(np.fft.ifft2(spec))
    return 0.5 + 0.42 * t / np.abs(t).max()


@functools.lru_cache(maxsize=None)
def film(depth, n, w=W, h=H):
    """n progressive film frames (Y, Cb, Cr): a vertically low-passed band-limited texture that moves 3 samples down and 5 across per frame (chroma: 1 and 2)"""
    peak = (1 << depth) - 1
    out = []
    for t in range(n):
        planes = []
        for k, (hh, ww, dy, dx) in enumerate(((h, w, 3, 5), (h // 2, w // 2, 1, 2), (h // 2, w // 2, 1, 2))):
            tex = _texture(100 + k, 256, 512, 1 / 24.0, 1 / 6.0)
            y0, x0 = (dy * t) % 256, (dx * t) % 512
            planes.append(np.ascontiguousarray(np.rint(np.roll(tex, (-y0, -x0), (0, 1))[:hh, :ww] * peak).astype(D.dtype(depth))))
        out.append(tuple(planes))
    return out


# ------------------------------------------------------------------------------------------------ clips
def pulldown_fields(n_frames, phase):
    """the film frame of every field of n_frames woven frames of 3:2 pulldown (film frames take 2, 3, 2, 3 ... fields), the clip beginning `phase` frames into
    the cycle of five: [(film of the first field in time, film of the second)]"""
    fields = []
    f = 0
    while len(fields) < 2 * (n_frames + phase):
        fields += [f] * (2 if f % 2 == 0 else 3)
        f += 1
    return [(fields[2 * (k + phase)], fields[2 * (k + phase) + 1]) for k in range(n_frames)]


def weave_fields(first, second, stored_tff):
    """one woven frame: the rows of the first field's parity from frame `first`, the others from `second`"""
    keep = 0 if stored_tff else 1
    return tuple(R.weave_plane(a, b, keep) for a, b in zip(first, second))


@functools.lru_cache(maxsize=None)
def telecined(depth, n_frames, phase, stored_tff=True, noise=0):
    """(frames, sources): n_frames woven frames of 3:2 pulldown over film(), and per frame the film frames of its (first, second) field.  noise: every sample
    moves by up to that many levels (8 bit; scaled with the depth), field by field, clamped"""
    src = pulldown_fields(n_frames, phase)
    fl = film(depth, max(b for _, b in src) + 1)
    frames = [weave_fields(fl[a], fl[b], stored_tff) for a, b in src]
    if noise:
        rng = np.random.default_rng(7 + phase)
        amp, peak = noise << (depth - 8), (1 << depth) - 1
        frames = [tuple(np.clip(p.astype(np.int64) + rng.integers(-amp, amp + 1, p.shape), 0, peak).astype(p.dtype) for p in f) for f in frames]
    return tuple(frames), tuple(src)


@functools.lru_cache(maxsize=None)
def hybrid(depth, n_frames=12, video=(5, 6, 7)):
    """(frames, video frames): a telecined clip whose frames `video` are true interlaced video: both fields of a frame come from different instants of a fast
    pan (the second field 11 samples further across), so no weave with a neighbour is clean"""
    frames, _ = telecined(depth, n_frames, 0)
    frames = list(frames)
    peak = (1 << depth) - 1
    for k in video:
        planes = []
        for i, (hh, ww) in enumerate(((H, W), (H // 2, W // 2), (H // 2, W // 2))):
            tex = _texture(200 + i, 256, 512, 1 / 24.0, 1 / 6.0)
            a = np.rint(np.roll(tex, -(22 * k), 1)[:hh, :ww] * peak).astype(D.dtype(depth))
            b = np.rint(np.roll(tex, -(22 * k + 11), 1)[:hh, :ww] * peak).astype(D.dtype(depth))
            planes.append(R.weave_plane(a, b, 0))
        frames[k] = tuple(planes)
    return tuple(frames), tuple(video)


def expected_film(sources, declared_tff, stored_tff):
    """per frame of a telecined clip: the film frame its KEPT field came from, and whether the other field of that film frame is in the frame, the one before or
    the one after (None: the clip does not hold it)"""
    out = []
    kept_is_first = declared_tff == stored_tff
    for k, (a, b) in enumerate(sources):
        f = a if kept_is_first else b

        def other(j):          # the film frame of the not-kept parity's field of frame j
            return (sources[j][1] if kept_is_first else sources[j][0]) if 0 <= j < len(sources) else None
        where = next((m for m, j in (("c", k), ("p", k - 1), ("n", k + 1)) if other(j) == f), None)
        out.append((f, where))
    return out


# ------------------------------------------------------------------------------------------------ kernel inputs
@functools.lru_cache(maxsize=None)
def frames(size, depth, kind):
    """(P, C, N): three frames of full-range noise (10 bit: values above the depth too), or three consecutive frames of a telecined clip of that size"""
    w, h = size
    if kind == "noise":
        return tuple(D.noise_frames(w, h, depth, w * h + depth + 1))
    fl = film(depth, 4, w, h)
    return (weave_fields(fl[0], fl[1], True), weave_fields(fl[1], fl[2], True), weave_fields(fl[3], fl[2], True))


@functools.lru_cache(maxsize=None)
def model_metrics(size, depth, kind, keep):
    P, C, N = frames(size, depth, kind)
    return R.metrics(P[0], C[0], N[0], depth, keep)


# ------------------------------------------------------------------------------------------------ GPU sessions
N_FRAMES = 12


def cfg_of(depth):
    cfg = base_cfg(depth)
    cfg.width, cfg.height = W, H
    return cfg


@functools.lru_cache(maxsize=None)
def clip(depth, tff, n=N_FRAMES):
    """the session clip: phase 1 (the first cycle holds no exact repeat of its own first frame), stored and declared with the same order"""
    return telecined(depth, n, 1, tff)[0]


@functools.lru_cache(maxsize=None)
def model_pictures(depth, tff, decimate, deint=True, n=N_FRAMES, which="clip"):
    """([(pts, display-size planes)], the plan) of a clip under the session's rules"""
    fr = list(clip(depth, tff, n) if which == "clip" else hybrid(depth)[0])
    pics, decided = R.pictures(fr, depth, tff, decimate, deint)
    return [(pts, [p[:H, :W] if i == 0 else p[:H // 2, :W // 2] for i, p in enumerate(planes)]) for pts, planes in pics], decided
