"""The scene-cut detector's sums (`k_scene_diff`, `mihevc_k_scene_diff`; DESIGN.md §5, the comment block of hevc_amd/csrc/gop_plan.h) as a plain numpy reference:
for n consecutive luma planes, out[i] = sum |a[y, x] - b[y, x]| over y, x = 0 (mod 4) inside width x height for the pair (i - 1, i), in int64; out[0] = 0.

Imports: numpy and the standard library only (tests/test_syntax_independent.py checks it)."""
import numpy as np


def scene_sums(planes, width, height):
    """planes: n arrays of at least height rows and width columns (anything beyond is pitch or padding and is not read) -> n Python ints"""
    out = [0]
    for a, b in zip(planes, planes[1:]):
        pa, pb = (np.asarray(p)[:height:4, :width:4].astype(np.int64) for p in (a, b))
        out.append(int(np.abs(pa - pb).sum()))
    return out


def sampled_positions(width, height):
    """how many positions one pair is summed over: ceil(width / 4) x ceil(height / 4)"""
    return -(-width // 4) * -(-height // 4)
