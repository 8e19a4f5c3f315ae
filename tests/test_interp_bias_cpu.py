"""CPU: the 8-bit fractional search's luma_half_diff (kernels/inter.h, stepped through tests/emu/interp.cpp) where its filtered rows carry no bias.
luma_row4_at returns hv' = sum of tap x (sample - 128), 128 * 64 less than the 14-bit-domain value, and every caller adds the bias back in a constant of
its own: the start value of the vertical sums (general path), the rounding constant (the two one-pass paths), luma_quad14's start value (motion
compensation).  Each path is held to source - weighted_uni(prediction) with the prediction from the spec-literal numpy form of 8.5.3.3.3.1 that the
independent decoder uses (tests/hevc_recon.py mc_luma, weighted_default), and to the same expression over the headers' own luma_quad14.  Every value
must be equal.

A 32 x 32 window, every (fx, fy): the 15 non-zero pairs take the general path; a zero fraction takes its one-pass path as a lone lane and the general
path as a lane of a mixed wave (common.h g_emu_mixed_wave), so both are run.  Contents: all 0, all 255, the two 0 / 255 checkerboards, 255 under the
positive taps with 0 under the negative ones and the inverse (per fraction: along the rows' taps, along the columns' taps, and by the sign of their
product), and seeded noise.  The 0 / 255 patterns are the ones that reach the limits of hv' (+14248 and -14312 of the 16 bits luma_col_pair packs)."""
import ctypes as C

import numpy as np
import pytest

from tests import hevc_recon as R
from tests import util

N, Y0, X0 = 32, 8, 8                         # the window's rows and row stride (a multiple of 4 samples), and the block's first integer sample in it
SLACK = 16                                   # samples behind the window, as the LDS image has them: a row's aligned dword reads may reach past its last sample


@pytest.fixture(scope="module")
def emu():
    return util.stepped_library()


def ptr(a, first=0):
    return C.c_void_p(a.ctypes.data + first * a.itemsize)


def tap_sign_windows(fx, fy, align):
    """255 where the tap that output (0, 0) of the block puts on the sample is positive, 0 where it is negative or zero -- along the row filter alone (every
    row alike: each filtered row is at its largest), along the column filter alone, and by the sign of the product of both -- and their inverses.  The
    patterns repeat with the taps' period of 8 samples."""
    kx = (np.arange(N) - (X0 + align - 3)) % 8
    ky = (np.arange(N) - (Y0 - 3)) % 8
    px, py = (R.FL[fx][kx] > 0), (R.FL[fy][ky] > 0)
    prod = (R.FL[fy][ky][:, None] * R.FL[fx][kx][None, :]) > 0
    out = []
    for on in (np.broadcast_to(px[None, :], (N, N)), np.broadcast_to(py[:, None], (N, N)), prod):
        out += [np.where(on, 255, 0), np.where(on, 0, 255)]
    return [w.astype(np.uint8) for w in out]


def plain_windows():
    y, x = np.mgrid[0:N, 0:N]
    return {"zero": np.zeros((N, N), np.uint8), "max": np.full((N, N), 255, np.uint8), "checker0": (((x + y) & 1) * 255).astype(np.uint8),
            "checker1": (((x + y + 1) & 1) * 255).astype(np.uint8), "noise": np.random.default_rng(20250).integers(0, 256, (N, N)).astype(np.uint8)}


def source(seed):
    src = np.random.default_rng(seed).integers(0, 256, (8, 32)).astype(np.uint8)
    src[::2] = 255 - src[::2] // 8           # differences of both signs and of full size against flat and checkerboard predictions
    src[1::2] //= 8
    return src


def held(win2d):
    """the window as the kernels hold it: 4-byte aligned, row stride N, slack behind the last row"""
    buf = np.zeros(N * N + SLACK, np.uint8)
    buf[:N * N] = win2d.ravel()
    assert buf.ctypes.data % 4 == 0
    return buf


def check(emu, win2d, align, fractions):
    src = source(31 + align)
    buf = held(win2d)
    x0, i00 = X0 + align, Y0 * N + X0 + align
    luma = np.zeros((16, 8, 4), np.int32)
    emu.emu_interp_luma14(ptr(buf), i00, N, 8, ptr(luma))
    one_pass, general = np.zeros((16, 8, 4), np.int32), np.zeros((16, 8, 4), np.int32)
    emu.emu_interp_half_diff(ptr(buf), i00, N, 8, ptr(src, 4), 32, 0, ptr(one_pass))     # a zero fraction takes its one-pass path
    emu.emu_interp_half_diff(ptr(buf), i00, N, 8, ptr(src, 4), 32, 1, ptr(general))      # every fraction takes the general path
    for fx, fy in fractions:
        f = fy * 4 + fx
        spec14 = R.mc_luma(win2d, x0, Y0, 8, (fx, fy), 8)[:, :4]
        assert np.array_equal(luma[f], spec14), ("luma_quad14", fx, fy)
        want = src[:, 4:8].astype(np.int64) - R.weighted_default([spec14], 8)
        own = src[:, 4:8].astype(np.int64) - R.weighted_default([luma[f].astype(np.int64)], 8)
        assert np.array_equal(own, want), ("own", fx, fy)
        assert np.array_equal(one_pass[f], want), ("lone lane", fx, fy)
        assert np.array_equal(general[f], want), ("mixed wave", fx, fy)


ALL = [(fx, fy) for fy in range(4) for fx in range(4)]


@pytest.mark.parametrize("align", range(4))
@pytest.mark.parametrize("kind", ["zero", "max", "checker0", "checker1", "noise"])
def test_half_diff_without_row_bias_plain_contents(emu, kind, align):
    check(emu, plain_windows()[kind], align, ALL)


@pytest.mark.parametrize("align", range(4))
def test_half_diff_without_row_bias_at_the_packing_limit(emu, align):
    for fx, fy in ALL:
        for win in tap_sign_windows(fx, fy, align):
            check(emu, win, align, [(fx, fy)])


def test_tap_sign_rows_reach_the_limits_of_the_unbiased_row():
    """what the patterns are for: a row of 255 under the positive taps filters to 255 * 88 (fraction 2: hv' = +14248 without the bias), its inverse to
    255 * -24 (hv' = -14312); both are inside the 16 bits of a packed pair, and 128 * 112 bounds every row"""
    pos = max(int(t[t > 0].sum()) for t in R.FL)
    neg = min(int(t[t < 0].sum()) for t in R.FL)
    assert (255 * pos - 128 * 64, 255 * neg - 128 * 64) == (14248, -14312)
    assert max(int(np.abs(t).sum()) for t in R.FL) == 112 and 128 * 112 < 1 << 15
    w = tap_sign_windows(2, 2, 0)
    row = w[0][Y0].astype(np.int64)
    assert int((R.FL[2] * row[X0 - 3:X0 + 5]).sum()) == 255 * pos
    row = w[1][Y0].astype(np.int64)
    assert int((R.FL[2] * row[X0 - 3:X0 + 5]).sum()) == 255 * neg
