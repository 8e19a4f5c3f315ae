"""CPU: the fractional-sample interpolation of kernels/inter.h, called directly (tests/emu/interp.cpp).  The sample primitives of motion compensation
(luma_quad14, chroma_sample14, weighted_uni) against the spec-literal numpy form of 8.5.3.3.3 / 8.5.3.3.4.2 that the independent decoder uses
(tests/hevc_recon.py mc_luma, mc_chroma, weighted_default), and the fractional search's luma_half_diff against source - weighted_uni(luma_quad14): the
search prices exactly the prediction that compensation writes.  Every start alignment of the window reads, every fraction, random, flat and checkerboard
contents at the ends of the sample range.  luma_half_diff runs twice: as a lone lane, where a zero fraction takes its one-pass path (horizontal-only,
vertical-only), and as a lane of a mixed wave (common.h g_emu_mixed_wave), where every fraction, zero ones too, takes the general two-pass path, which
otherwise meets a zero fraction only on the device; the two must agree.  Then the LDS layouts of the two CTU kernels at me_range 15."""
import ctypes as C

import numpy as np
import pytest

from tests import hevc_recon as R
from tests import util

ROWS, Y0, X0 = 24, 8, 8                      # the window's rows, and the block's first integer sample in it (start alignment added to X0)
CONTENTS = ["random", "zero", "max", "checker0", "checker1"]


@pytest.fixture(scope="module")
def emu():
    lib = util.stepped_library()
    lib.emu_weighted_uni.restype = C.c_int
    return lib


@pytest.fixture(scope="module")
def stride(emu):
    out = (C.c_longlong * 13)()
    emu.emu_inter_layout(1, 8, out)
    return int(out[12])                      # mc_win_y_stride(8)


def window(kind, bd, ws, seed):
    maxv, dt = (1 << bd) - 1, np.uint8 if bd == 8 else np.uint16
    y, x = np.mgrid[0:ROWS, 0:ws]
    if kind == "random":
        return np.random.default_rng(seed).integers(0, maxv + 1, (ROWS, ws)).astype(dt)
    if kind in ("zero", "max"):
        return np.full((ROWS, ws), maxv if kind == "max" else 0, dt)
    return (((x + y + int(kind[-1])) & 1) * maxv).astype(dt)


def cases():
    return [(bd, a, kind) for bd in (8, 10) for a in range(4 if bd == 8 else 2) for kind in CONTENTS]


def ptr(a, first=0):
    return C.c_void_p(a.ctypes.data + first * a.itemsize)


@pytest.mark.parametrize("bd,align,kind", cases())
def test_sample_primitives_equal_the_spec_form(emu, stride, bd, align, kind):
    win = np.ascontiguousarray(window(kind, bd, stride, 100 * bd + align))
    assert win.ctypes.data % 4 == 0
    x0, i00 = X0 + align, Y0 * stride + X0 + align
    luma = np.zeros((16, 8, 4), np.int32)
    emu.emu_interp_luma14(ptr(win), i00, stride, bd, ptr(luma))
    chroma = np.zeros((64, 4, 4), np.int32)
    emu.emu_interp_chroma14(ptr(win), i00, stride, bd, ptr(chroma))
    for f in range(16):
        want = R.mc_luma(win, x0, Y0, 8, (f & 3, f >> 2), bd)[:, :4]
        assert np.array_equal(luma[f], want), (f & 3, f >> 2)
    for f in range(64):
        want = R.mc_chroma(win, x0, Y0, 4, (f & 7, f >> 3), bd)
        assert np.array_equal(chroma[f], want), (f & 7, f >> 3)
    for v14 in (luma, chroma):
        vals = np.unique(v14)
        got = np.array([emu.emu_weighted_uni(int(p), bd) for p in vals])
        assert np.array_equal(got, R.weighted_default([vals.astype(np.int64)], bd))


@pytest.mark.parametrize("bd,align,kind", cases())
def test_search_prices_the_compensated_prediction(emu, stride, bd, align, kind):
    win = np.ascontiguousarray(window(kind, bd, stride, 100 * bd + align))
    maxv = (1 << bd) - 1
    src = np.random.default_rng(7 * bd + align).integers(0, maxv + 1, (8, 32)).astype(win.dtype)
    if kind != "random":
        src[::2] = maxv - src[::2] // 8      # differences of both signs and of full size against flat and checkerboard predictions
        src[1::2] //= 8
    x0, i00 = X0 + align, Y0 * stride + X0 + align
    luma = np.zeros((16, 8, 4), np.int32)
    emu.emu_interp_luma14(ptr(win), i00, stride, bd, ptr(luma))
    uni = {int(p): emu.emu_weighted_uni(int(p), bd) for p in np.unique(luma)}
    own = src[:, 4:8].astype(np.int64) - np.vectorize(uni.get)(luma)         # source - weighted_uni(luma_quad14), by the headers themselves
    one_pass, general = np.zeros((16, 8, 4), np.int32), np.zeros((16, 8, 4), np.int32)
    emu.emu_interp_half_diff(ptr(win), i00, stride, bd, ptr(src, 4), 32, 0, ptr(one_pass))     # a zero fraction takes its one-pass path
    emu.emu_interp_half_diff(ptr(win), i00, stride, bd, ptr(src, 4), 32, 1, ptr(general))      # every fraction, zero ones too, takes the general path
    for f in range(16):
        fx, fy = f & 3, f >> 2
        want = src[:, 4:8].astype(np.int64) - R.weighted_default([R.mc_luma(win, x0, Y0, 8, (fx, fy), bd)[:, :4]], bd)
        assert np.array_equal(own[f], want), (fx, fy)
        assert np.array_equal(one_pass[f], want), (fx, fy)
        assert np.array_equal(general[f], want), (fx, fy)
        assert np.array_equal(general[f], one_pass[f]), (fx, fy)


def test_lds_layouts_at_8_bit_me_range_15(emu):
    """the numbers of the build before the layouts moved into mc_win_*_bytes / inter_b_lds: k_inter_ctu keeps its 31,440 bytes (5 workgroups per CU) with
    the luma window inside rs.scratch (the Y_IN kernel), k_inter_ctu_b its 43,248"""
    out = (C.c_longlong * 13)()
    emu.emu_inter_layout(1, 15, out)
    win_y, win_c, y, u, v, total, y_in, by, bu, bv, bbi, btotal, _ = [int(x) for x in out]
    assert (win_y, win_c) == (6096, 2128)
    assert (y, u, v, total, y_in) == (14656, 20752, 29312, 31440, 1)
    assert (by, bu, bv, bbi, btotal) == (29312, 35408, 37536, 39664, 43248)
    emu.emu_inter_layout(2, 15, out)         # Main10: the luma window behind InterShared
    assert [int(x) for x in out[:12]] == [12192, 4256, 32384, 14656, 18912, 44576, 0, 32384, 44576, 48832, 53088, 56672]
