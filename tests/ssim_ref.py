"""numpy reference of the per-picture SSIM a session reports with cfg.ssim (hevc_amd/csrc/kernels/ssim.h states the same five steps).
numpy and the standard library only: neither the oracle nor the package is imported here.

For one colour component, a = source, b = reconstruction, both of the coded size (multiples of 4), peak = 2^bitDepth - 1:
 1. 4x4 blocks on the 4-sample grid: s1 = sum a, s2 = sum b, ss = sum (a^2 + b^2), s12 = sum a b
 2. a window = 2x2 adjacent blocks (8x8 samples, stride 4): (W/4 - 1)(H/4 - 1) windows, its sums are the four blocks' sums
 3. int64: vars = 64 ss - s1^2 - s2^2, covar = 64 s12 - s1 s2, c1 = (4096 peak^2 + 5000) // 10000, c2 = (9 * 4096 peak^2 + 5000) // 10000,
    f1 = 2 s1 s2 + c1, f2 = 2 covar + c2, g1 = s1^2 + s2^2 + c1, g2 = vars + c2 (all below 2^53: exact as float64)
 4. q = (float64(f1) * float64(f2)) / (float64(g1) * float64(g2)); Q = rint(q * 2^32) as int64 (ties to even)
 5. the picture's value: the int64 sum of Q and the window count; SSIM = sum / (windows * 2^32)
"""
import numpy as np

ONE = 1 << 32


def constants(bit_depth):
    """(c1, c2): (0.01 peak)^2 and (0.03 peak)^2 scaled by 64^2, rounded"""
    peak = (1 << bit_depth) - 1
    return (4096 * peak * peak + 5000) // 10000, (9 * 4096 * peak * peak + 5000) // 10000


def window_count(w, h):
    return (w // 4 - 1) * (h // 4 - 1)


def window_sums(a, b):
    """(s1, s2, ss, s12) per window, int64 arrays of shape (H/4 - 1, W/4 - 1)"""
    a, b = np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64)
    h, w = a.shape
    assert a.shape == b.shape and h % 4 == 0 and w % 4 == 0 and h >= 8 and w >= 8, (a.shape, b.shape)

    def blocks(x):
        return x.reshape(h // 4, 4, w // 4, 4).sum(axis=(1, 3))

    def windows(x):
        return x[:-1, :-1] + x[:-1, 1:] + x[1:, :-1] + x[1:, 1:]
    return tuple(windows(blocks(x)) for x in (a, b, a * a + b * b, a * b))


def terms(s1, s2, ss, s12, bit_depth):
    """(f1, f2, g1, g2) of step 3, int64"""
    c1, c2 = constants(bit_depth)
    var = 64 * ss - s1 * s1 - s2 * s2
    covar = 64 * s12 - s1 * s2
    return 2 * s1 * s2 + c1, 2 * covar + c2, s1 * s1 + s2 * s2 + c1, var + c2


def window_q32(a, b, bit_depth):
    """Q of every window: int64 array of shape (H/4 - 1, W/4 - 1)"""
    f1, f2, g1, g2 = terms(*window_sums(a, b), bit_depth)
    for t in (f1, f2, g1, g2):
        assert np.abs(t).max() < 1 << 53
    q = (f1.astype(np.float64) * f2.astype(np.float64)) / (g1.astype(np.float64) * g2.astype(np.float64))
    return np.rint(q * float(ONE)).astype(np.int64)


def plane(a, b, bit_depth):
    """(int64 sum of Q, window count) of one component"""
    q = window_q32(a, b, bit_depth)
    return int(q.sum(dtype=np.int64)), int(q.size)


def picture(src, rec, bit_depth):
    """src, rec: (y, u, v) planes of the coded size -> ([sum_q32] * 3, [windows] * 3)"""
    r = [plane(a, b, bit_depth) for a, b in zip(src, rec)]
    return [x[0] for x in r], [x[1] for x in r]


def value(sum_q32, windows):
    return sum_q32 / (windows * float(ONE))


def extend(p, w, h):
    """a display-size plane extended to w x h by edge replication, as a session extends its source"""
    p = np.asarray(p)
    return np.pad(p, ((0, h - p.shape[0]), (0, w - p.shape[1])), mode="edge")
