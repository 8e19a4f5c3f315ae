"""What the tests of the downscaling source (test_scale_cpu, test_gpu_scale and its child process scale_device_child) share: the size pairs and depths, their
random sources and model outputs, computed once, and the small sessions of the GPU tests."""
import functools

from tests import scale_ref as R
from tests import util
from tests.ingest_common import H, N, W, base_cfg

# (source size, output size): 1:1, 3:2, 2:1, 4:1, 2:1 by 1:1 and an uneven ratio onto 136x72 (coded size = display size, more than one tile each way);
# the same onto 70x38 (a margin on both sides, a chroma row that ends with half a run; 3:2 of it is 105x57, so the nearest even size stands in)
CASES = [((136, 72), (136, 72)), ((204, 108), (136, 72)), ((272, 144), (136, 72)), ((544, 288), (136, 72)), ((272, 72), (136, 72)), ((262, 106), (136, 72)),
         ((70, 38), (70, 38)), ((106, 58), (70, 38)), ((140, 76), (70, 38)), ((280, 152), (70, 38)), ((140, 38), (70, 38))]
DEPTHS = [(b, d) for b in (8, 10, 16) for d in (8, 10)]


def case_id(c):
    return f"{c[0][0]}x{c[0][1]}-{c[1][0]}x{c[1][1]}"


@functools.lru_cache(maxsize=None)
def source(case, B):
    (sw, sh), _ = case
    return R.random_source(sw, sh, B, sw * sh + B, full_word=True)


@functools.lru_cache(maxsize=None)
def model(case, B, D):
    return R.scale(*source(case, B), B, *case[1], D)


# ------------------------------------------------------------------------------------------------ GPU sessions (100x70, 5 pictures: ingest_common)
SOURCES = [(200, 140), (150, 104), (400, 280)]
OTHER = (136, 72)             # a second session's size


@functools.lru_cache(maxsize=None)
def clip(size, depth):
    """N pictures of a translating scene of `size` at `depth` bits"""
    sw, sh = size
    return [util.planes(util.synth_frame(sh, sw, seed=3, shift=(4 * i, 2 * i), bit_depth=depth), depth) for i in range(N)]


def cfg_of(depth, w=W, h=H):
    cfg = base_cfg(depth)
    cfg.width, cfg.height = w, h
    return cfg
