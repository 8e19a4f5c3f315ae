"""What the tests of the upscaling source (test_upscale_cpu, test_gpu_upscale and its child process upscale_device_child) share: the size pairs, depths and
settings, their random sources and model outputs, computed once, and the small sessions of the GPU tests."""
import functools

from tests import upscale_ref as R
from tests import util
from tests.ingest_common import H, N, W, base_cfg
from tests.scale_common import DEPTHS      # noqa: F401 (the depth pairs are the downscaler's)

# (source size, output size): 1:1, about 3:2, 2:1, 4:1 (chroma 17x9), 2:1 by 1:1 and an uneven ratio onto 136x72 (coded size = display size, more than one tile
# each way); then 1:1, about 3:2, about 2:1 and about 4:1 onto 70x38 (a margin on both sides, a chroma row that ends with half a run)
CASES = [((136, 72), (136, 72)), ((90, 48), (136, 72)), ((68, 36), (136, 72)), ((34, 18), (136, 72)), ((68, 72), (136, 72)), ((50, 26), (136, 72)),
         ((70, 38), (70, 38)), ((46, 26), (70, 38)), ((36, 20), (70, 38)), ((18, 16), (70, 38))]
SETTINGS = [(0, 0), (0, 8), (8, 8), (64, 5)]          # (sharpen, antiring)


def case_id(c):
    return f"{c[0][0]}x{c[0][1]}-{c[1][0]}x{c[1][1]}"


@functools.lru_cache(maxsize=None)
def source(case, B):
    (sw, sh), _ = case
    return R.random_source(sw, sh, B, sw * sh + B, full_word=True)


@functools.lru_cache(maxsize=None)
def model(case, B, D, setting):
    return R.upscale(*source(case, B), B, *case[1], D, *setting)


# ------------------------------------------------------------------------------------------------ GPU sessions (100x70, 5 pictures: ingest_common)
SOURCES = [(50, 36), (68, 48), (26, 18)]


@functools.lru_cache(maxsize=None)
def clip(size, depth):
    """N pictures of a translating scene of `size` at `depth` bits: the top left corner of a scene of at least 48x40, the smallest util.synth_frame draws"""
    import numpy as np
    sw, sh = size
    frames = [util.planes(util.synth_frame(max(sh, 40), max(sw, 48), seed=3, shift=(4 * i, 2 * i), bit_depth=depth), depth) for i in range(N)]
    return [tuple(np.ascontiguousarray(p[:h, :w]) for p, (w, h) in zip(f, ((sw, sh), (sw // 2, sh // 2), (sw // 2, sh // 2)))) for f in frames]


def cfg_of(depth, w=W, h=H):
    cfg = base_cfg(depth)
    cfg.width, cfg.height = w, h
    return cfg
