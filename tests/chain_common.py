"""What the tests of the source filter chain share (test_chain_cpu, test_gpu_chain and its child process chain_device_child): the sizes, the clips built from the
generators of the single filters' tests, the chains of the cases and their models, computed once, and the small sessions of the GPU tests."""
import functools

import numpy as np

from tests import chain_ref as CR
from tests import deint_ref, denoise_ref
from tests.fieldmatch_common import film, pulldown_fields, weave_fields
from tests.ingest_common import base_cfg

# a 52x36 source into a 100x68 session (coded 104x72: the margin fill, and 25 : 13 and 17 : 9 are no integer ratios) for the chains that enlarge, 200x136 into
# 100x68 for those that reduce, 100x68 throughout where no resize stage is on.  Every generator used takes these sizes as they are
SMALL, SESSION, LARGE = (52, 36), (100, 68), (200, 136)
N_FRAMES = 12          # two cycles of inverse telecine and a partial one


def cfg_of(depth, size=SESSION):
    cfg = base_cfg(depth)
    cfg.width, cfg.height = size
    return cfg


@functools.lru_cache(maxsize=None)
def clip(kind, size, depth, n=N_FRAMES):
    """n frames (Y, Cb, Cr).  telecine: 3:2 pulldown, phase 1, top field first, over the moving film frames of tests/fieldmatch_common.py, every sample moved by
    up to 2 levels (8 bit) of noise; film: those film frames themselves with the same noise (a pair of them moves by (5, 3)); interlaced: the woven frames of
    tests/deint_ref.py; noisy: the noisy frames of tests/denoise_ref.py"""
    w, h = size
    if kind == "interlaced":
        return tuple(deint_ref.woven_frames(w, h, depth, n, tff=True, seed=11 + depth))
    if kind == "noisy":
        return tuple(denoise_ref.noisy_frames(w, h, depth, n, 3, seed=11 + depth)[0])
    if kind == "telecine":
        src = pulldown_fields(n, 1)
        fl = film(depth, max(b for _, b in src) + 1, w, h)
        frames = [weave_fields(fl[a], fl[b], True) for a, b in src]
    else:
        assert kind == "film"
        frames = film(depth, n, w, h)
    rng = np.random.default_rng(7 + w + depth)
    amp, peak = 2 << (depth - 8), (1 << depth) - 1
    return tuple(tuple(np.ascontiguousarray(np.clip(p.astype(np.int64) + rng.integers(-amp, amp + 1, p.shape), 0, peak).astype(p.dtype)) for p in f) for f in frames)


# name: (clip kind, source size, chain)
ONE_SLOT = {
    "deint-frame": ("interlaced", SESSION, dict(field="deint", tff=True, field_rate=False)),
    "deint-field": ("interlaced", SESSION, dict(field="deint", tff=True, field_rate=True)),
    "ivtc": ("telecine", SESSION, dict(field="fieldmatch", tff=True, decimate=True)),
    "match": ("telecine", SESSION, dict(field="fieldmatch", tff=True, decimate=False)),
    "denoise": ("noisy", SESSION, dict(denoise=2)),
    "scale": ("noisy", LARGE, dict(resize="scale", size=SESSION)),
    "upscale": ("noisy", SMALL, dict(resize="upscale", size=SESSION, sharpen=8, antiring=8)),
    "interpolate": ("film", SESSION, dict(interpolate=2)),
}
TWO_SLOT = {
    "deint-scale": ("interlaced", LARGE, dict(field="deint", tff=True, field_rate=False, resize="scale", size=SESSION)),
    "bob-interp2": ("interlaced", SESSION, dict(field="deint", tff=True, field_rate=True, interpolate=2)),
    "ivtc-denoise": ("telecine", SESSION, dict(field="fieldmatch", tff=True, decimate=True, denoise=2)),
    "denoise-upscale": ("noisy", SMALL, dict(denoise=2, resize="upscale", size=SESSION)),
    "upscale-interp3": ("film", SMALL, dict(resize="upscale", size=SESSION, interpolate=3)),
}
FULL = ("telecine", SMALL, dict(field="fieldmatch", tff=True, decimate=True, fm_deint=True, denoise=2, resize="upscale", size=SESSION, interpolate=2))
MULTI = {**TWO_SLOT, "full": FULL}


@functools.lru_cache(maxsize=None)
def _model(kind, size, depth, out_depth, n, items, with_plan):
    chain = dict(items)
    if chain.get("resize") is not None:
        chain["out_depth"] = out_depth
    return CR.pictures(list(clip(kind, size, depth, n)), depth, chain, with_plan)


def model(case, depth, out_depth=None, n=N_FRAMES, chain=None, with_plan=False):
    """[(pts, display-size planes)] of a case (clip kind, source size, chain) at `depth`; out_depth: the session's (None: the source's); chain: another chain
    over the same clip"""
    kind, size, own = case
    return _model(kind, size, depth, out_depth or depth, n, tuple(sorted((own if chain is None else chain).items(), key=str)), with_plan)


def lib_kwargs(chain):
    """the keywords of hevc_amd._lib.chain / Encoder.set_chain for a chain of tests/chain_ref.py"""
    return {k: v for k, v in chain.items() if k not in ("size", "out_depth")}


def session_size(case):
    return case[2].get("size", case[1])
