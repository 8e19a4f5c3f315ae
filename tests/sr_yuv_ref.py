"""numpy model of the Y'CbCr input of the learned super-resolution (mihevc_send_frame_sr_yuv / mihevc_k_sr_from_yuv), written from DESIGN.md §6l; imports nothing
from hevc_amd and shares nothing with the kernel header.  Steps 1 and 2 are those of the colour table (§6i), taken from tests/lut3d_ref.py, which states them on
its own; the half conversion is the one tests/sr_common.py's input_want uses (tests/sr_ref.py input_tensor).

  source   W x H, both even; planar 4:2:0 at B = 8, 10 or 12 bit, v = min(r, 2^B - 1); matrix 1, 5, 6 or 9; limited or full range
  1, 2     chroma to the luma grid with the factor 8, then R'G'B' at 16 bit, v = clip((t + 2^15) >> 16, 0, 65535)
  3        x = half(float32(v) / float32(65535))
  tensor   scale 4: [H, W, 32], channels 0 .. 2 = R, G, B; scale 2: [H/2, W/2, 32], channel c 4 + dy 2 + dx at (y, x) = component c at (2y + dy, 2x + dx);
           every other channel zero
"""
import numpy as np

from tests import lut3d_ref as L
from tests import sr_ref as R


def clamped(planes, B):
    return [np.minimum(np.asarray(p, np.int64), (1 << B) - 1) for p in planes]


def rgb16(planes, B, matrix, full, grid=L.chroma_to_luma_grid):
    """[3, H, W] int64: R', G', B' at 16 bit.  grid: step 1 (the tests pass a variant without a clamp to see what an edge case is worth)"""
    y, u, v = clamped(planes, B)
    return np.stack(L.to_rgb16(y, grid(u), grid(v), matrix, full, B))


def tensor_of_rgb16(rgb, scale):
    """[3, H, W] values 0 .. 65535 -> the input tensor as half bits, [th, tw, 32] uint16"""
    x = R.input_tensor(list(rgb), 65535)                # [3, H, W] float16
    if scale == 2:
        c, h, w = x.shape
        u = np.zeros((4 * c, h // 2, w // 2), np.float16)
        for comp in range(c):
            for dy in range(2):
                for dx in range(2):
                    u[comp * 4 + dy * 2 + dx] = x[comp, dy::2, dx::2]
        x = u
    out = np.zeros(x.shape[1:] + (32,), np.float16)
    out[:, :, :x.shape[0]] = x.transpose(1, 2, 0)
    return np.ascontiguousarray(out).view(np.uint16)


def input_tensor(planes, B, matrix, full, scale, grid=L.chroma_to_luma_grid):
    return tensor_of_rgb16(rgb16(planes, B, matrix, full, grid), scale)


def grid_without(clamp):
    """step 1 with one clamp dropped: the neighbour past that edge is the sample an unclamped index would reach by wrapping round, not the edge's own.
    clamp: 'right' (column W/2 - 1), 'top' (row 0), 'bottom' (row H/2 - 1)"""
    def grid(c):
        c = np.asarray(c, np.int64)
        right = np.roll(c, -1, axis=1) if clamp == "right" else np.concatenate([c[:, 1:], c[:, -1:]], axis=1)
        h = np.empty((c.shape[0], 2 * c.shape[1]), np.int64)
        h[:, 0::2] = 2 * c
        h[:, 1::2] = c + right
        up = np.roll(h, 1, axis=0) if clamp == "top" else np.concatenate([h[:1], h[:-1]])
        down = np.roll(h, -1, axis=0) if clamp == "bottom" else np.concatenate([h[1:], h[-1:]])
        out = np.empty((2 * h.shape[0], h.shape[1]), np.int64)
        out[0::2] = 3 * h + up
        out[1::2] = 3 * h + down
        return out
    return grid
