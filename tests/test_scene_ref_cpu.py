"""CPU: tests/scene_ref.py, the numpy statement of the scene-cut detector's sums, pinned by hand; and what mihevc_k_scene_diff refuses before it touches a
device.  tests/test_gpu_scene_diff.py holds the kernel to the reference."""
import ctypes as C

import numpy as np

from hevc_amd import _lib
from tests import scene_ref as S
from tests import util


def test_one_sampled_and_one_unsampled_position():
    """two 8x8 pictures: the sampled positions are (0, 0), (0, 4), (4, 0), (4, 4).  They differ by 9 at (4, 4), which is one of them, and by 200 at (5, 4),
    which is not: the sum is 9"""
    a = np.full((8, 8), 50, np.uint8)
    b = a.copy()
    b[4, 4], b[5, 4] = 41, 250
    assert S.scene_sums([a, b], 8, 8) == [0, 9] and S.scene_sums([b, a], 8, 8) == [0, 9]
    assert S.scene_sums([a, b, b, a], 8, 8) == [0, 9, 0, 9] and S.scene_sums([a], 8, 8) == [0]
    assert S.sampled_positions(8, 8) == 4


def test_flat_pairs_and_sizes_that_are_no_multiple_of_four():
    """all 0 against all 1023: 1023 per sampled position, ceil(w / 4) x ceil(h / 4) of them"""
    for w, h in ((8, 8), (9, 5), (10, 6), (11, 7), (12, 8), (136, 72), (1, 1)):
        a, b = np.zeros((h, w), np.uint16), np.full((h, w), 1023, np.uint16)
        assert S.scene_sums([a, b], w, h) == [0, 1023 * -(-w // 4) * -(-h // 4)], (w, h)
    assert S.sampled_positions(9, 5) == 3 * 2 and S.sampled_positions(1920, 1080) == 129600
    # what lies beyond width x height (the pitch, rows of padding) is not read
    a, b = np.zeros((12, 16), np.uint8), np.zeros((12, 16), np.uint8)
    b[:, 5:] = 255
    b[5:, :] = 255
    assert S.scene_sums([a, b], 5, 5) == [0, 0] and S.scene_sums([a, b], 9, 5) == [0, 2 * 255] and S.scene_sums([a, b], 9, 9) == [0, 255 * 5]


def test_the_entry_refuses_bad_arguments_before_any_device_call():
    lib = _lib.load()
    z = np.zeros((8, 16), np.uint8)
    for planes, w, h, bd, pitches in (([], 8, 8, 8, None),                       # n = 0
                                      ([z, z], 8, 8, 9, None), ([z, z], 8, 8, 12, None),
                                      ([z, z], 17, 8, 8, None),                  # pitch 16 < width 17
                                      ([z, z], 8, 8, 8, [16, 7]),
                                      ([z, z], 0, 8, 8, None), ([z, z], 8, 0, 8, None)):
        assert util.scene_diff(lib, planes, w, h, bd, device=0, pitches=pitches)[0] == _lib.EINVAL, (len(planes), w, h, bd, pitches)
    ptrs, pitch, out = (C.c_void_p * 2)(z.ctypes.data, None), (C.c_int32 * 2)(16, 16), (C.c_uint64 * 2)()
    assert lib.mihevc_k_scene_diff(0, ptrs, pitch, 2, 8, 8, 8, out) == _lib.EINVAL       # a null plane
    assert lib.mihevc_k_scene_diff(0, None, pitch, 2, 8, 8, 8, out) == _lib.EINVAL
    assert lib.mihevc_k_scene_diff(0, ptrs, pitch, -1, 8, 8, 8, out) == _lib.EINVAL
