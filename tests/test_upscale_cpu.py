"""CPU: the upscaling source (mihevc_send_frame_upscaled / mihevc_k_upscale_source).  The numpy model of tests/upscale_ref.py against hand-worked
cases and a scalar restatement in Python ints; its properties; the table builder of hevc_amd/csrc/scale_taps.h against the model's Fraction tables, row for row;
the kernel program of hevc_amd/csrc/kernels/upscale.h stepped on the CPU (tests/emu/upscale.cpp) against the model, bit for bit, over random initial LDS in the
three lane orders; the sanitizer program; the new entry points without a device; the ABI struct; upscale_target and encode_file(upscale=) in front of a stand-in
ffmpeg."""
import ctypes as C
import json
import math
import subprocess
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

from hevc_amd import _lib
from tests import scale_ref as SR
from tests import upscale_ref as R
from tests import util
from tests.ingest_common import fake_ffmpeg, info, same_planes      # noqa: F401 (fake_ffmpeg: a fixture)
from tests.upscale_common import CASES, DEPTHS, SETTINGS, SOURCES, case_id, model, source

ROOT = Path(__file__).resolve().parents[1]
SETTING_IDS = [f"s{g}a{ar}" for g, ar in SETTINGS]


# ------------------------------------------------------------------------------------------------ 1. the model against hand-worked cases
def test_model_two_to_one_rows():
    # centre aligned 1:2: pos = i/2 - 1/4.  Even i: taps k = i/2 - 2 .. i/2 + 1 at |t| = 1.75, 0.75, 0.25, 1.25: CR = -3/128, 29/128, 111/128, -9/128; c = CR * 4096.
    # Odd i: the mirror image from k = (i - 1)/2 - 1
    first, near, coef, longest = R.table(16, 32, 2)
    assert longest == 4
    for i in range(0, 32, 2):
        assert first[i] == i // 2 - 2 and near[i] == i // 2 - 1 and coef[i].tolist() == [-96, 928, 3552, -288]
        assert first[i + 1] == i // 2 - 1 and near[i + 1] == i // 2 and coef[i + 1].tolist() == [-288, 3552, 928, -96]


def test_model_one_to_one_is_a_single_tap():
    for p in (1, 2):
        first, near, coef, longest = R.table(40, 40, p)
        assert longest == 1 and first.tolist() == near.tolist() == list(range(40)) and np.all(coef[:, 0] == 4096) and not coef[:, 1:].any()


def test_model_one_to_three_has_a_row_that_starts_later():
    # 1:3 centre aligned: pos = (i - 1) / 3: every third output sample sits on a source sample and keeps one tap, which starts one sample after the four of the
    # row that follows it: `first` is not monotone, `near` is
    first, near, coef, longest = R.table(16, 48, 2)
    assert longest == 4 and first[:4].tolist() == [-2, 0, -1, -1] and near[:4].tolist() == [-1, 0, 0, 0] and coef[1].tolist() == [4096, 0, 0, 0]
    assert np.all(np.diff(near) >= 0) and not np.all(np.diff(first) >= 0)


def test_model_edge_column_and_both_signs_of_overshoot():
    # 1:2, 8 bit -> 8 bit (G = 4: m = (sum + 128) >> 8 in sixteenths, P = (t' + 8) >> 4), column 0 is 200 and the rest 0, every row equal, so the vertical pass
    # returns m' (one value times 4096) and its blend changes nothing.
    #   i = 0 (pos -1/4, near -1, taps -2 .. 1, three of them read column 0): (-96 + 928 + 3552) * 200 = 876800 -> m = 3425; a = b = 200: lo = hi = 3200
    #          ar 0: 3425 -> 214;  ar 8: 3200 -> 200;  ar 5: 3425 + floor((-225 * 5 + 4) / 8) = 3425 - 141 = 3284 -> 205
    #   i = 1 (pos 1/4, near 0, taps -1 .. 2): (-288 + 3552) * 200 = 652800 -> 2550, inside [0, 3200] -> 159
    #   i = 2 (pos 3/4, near 0): (-96 + 928) * 200 -> 650 -> 41
    #   i = 3 (pos 5/4, near 1): -288 * 200 -> floor(-224.5) = -225; a = b = 0: ar 8 lifts it to 0, ar 0 leaves -225 -> floor(-13.6) = -14, clamped to 0 at the end
    y = np.zeros((16, 16), np.uint8)
    y[:, 0] = 200
    c = np.zeros((8, 8), np.uint8)
    for ar, head in ((0, [214, 159, 41, 0, 0]), (8, [200, 159, 41, 0, 0]), (5, [205, 159, 41, 0, 0])):
        out = R.upscale(y, c, c, 8, 32, 32, 8, 0, ar)[0]
        assert out[7, :5].tolist() == head and not out[:, 3:].any() and np.all(out == out[0])
    v = y.astype(np.int64)
    m = (R.filter_axis(v, 16, 32, 2, 1) + 128) >> 8
    assert m[3, :5].tolist() == [3425, 2550, 650, -225, -75]
    assert R.blend_to_range(m, v, 16, 32, 2, 1, 16, 8)[3, :5].tolist() == [3200, 2550, 650, 0, 0]
    assert R.blend_to_range(m, v, 16, 32, 2, 1, 16, 5)[3, :5].tolist() == [3284, 2550, 650, -84, -28]      # -225 + floor((225 * 5 + 4) / 8) = -225 + 141
    # the same picture turned: the vertical pass meets the same numbers on m' = 16 v
    out = R.upscale(np.ascontiguousarray(y.T), c, c, 8, 32, 32, 8, 0, 8)[0]
    assert out[:5, 9].tolist() == [200, 159, 41, 0, 0]


def test_model_sharpener_by_hand():
    # a corner sample, its neighbours clamped into the plane: the 3x3 of sample (0, 0) of [[50, 60], [40, 20]] is [[50, 50, 60], [50, 50, 60], [40, 40, 20]]:
    # e = 50 + 50 + 60 + 40 = 200, f = 50 + 60 + 40 + 20 = 170, d16 = 800 - (200 + 400 + 170) = 30; g 64: 50 + (1920 + 128 >> 8) = 58; g 16: 50 + (608 >> 8) = 52
    P = np.array([[50, 60], [40, 20]])
    assert R.sharpen_plane(P, 64)[0, 0] == 58 and R.sharpen_plane(P, 16)[0, 0] == 52 and np.array_equal(R.sharpen_plane(P, 0), P)
    # a sample that hits its min3x3: centre 70 among 80s and one 60: e = 320, f = 300, d16 = 1120 - (280 + 640 + 300) = -100;
    # g 64: 70 + floor((-6400 + 128) / 256) = 70 - 25 = 45 -> 60, the smallest of the nine; g 8: 70 + floor(-672 / 256) = 67
    P = np.array([[80, 80, 80], [80, 70, 80], [80, 80, 60]])
    assert R.sharpen_plane(P, 64)[1, 1] == 60 and R.sharpen_plane(P, 8)[1, 1] == 67
    # and one that hits its max3x3: a corner of 100 above smaller neighbours
    assert R.sharpen_plane(np.array([[100, 60], [40, 20]]), 16)[0, 0] == 100


# ------------------------------------------------------------------------------------------------ 2. a scalar restatement in Python ints
def scalar_axis(S, Dn, p):
    """[(near, {k: c})] per output sample, from the definition"""
    rows = []
    for i in range(Dn):
        pos = Fraction((4 * i + p) * S - p * Dn, 4 * Dn)
        ks = [k for k in range(math.floor(pos) - 3, math.floor(pos) + 4) if abs(pos - k) < 2]
        w = [SR.cr(pos - k) for k in ks]
        c = [math.floor(x * 4096 / sum(w) + Fraction(1, 2)) for x in w]
        c[c.index(max(c))] += 4096 - sum(c)
        rows.append((math.floor(pos), dict(zip(ks, c))))
    return rows


def scalar_blend(x, a, b, ar):
    return x + ((min(max(x, min(a, b)), max(a, b)) - x) * ar + 4 >> 3)


def scalar_upscale(planes, B, dw, dh, D, g, ar):
    G = min(4, 16 - B)
    n, u = G + max(0, B - D), max(0, D - B)
    out = []
    for c, pl in enumerate(planes):
        S_h, S_w = pl.shape
        w, h = (dw, dh) if c == 0 else (dw // 2, dh // 2)
        v = [[min(int(x), (1 << B) - 1) for x in r] for r in pl]
        hx, vx = scalar_axis(S_w, w, 2 if c == 0 else 1), scalar_axis(S_h, h, 2)
        cl = lambda k, S: min(max(k, 0), S - 1)      # noqa: E731
        mm = [[scalar_blend((sum(cf * r[cl(k, S_w)] for k, cf in taps.items()) + (1 << (11 - G))) >> (12 - G), r[cl(nr, S_w)] << G, r[cl(nr + 1, S_w)] << G, ar)
               for nr, taps in hx] for r in v]
        P = [[0] * w for _ in range(h)]
        for j, (nr, taps) in enumerate(vx):
            for i in range(w):
                t = (sum(cf * mm[cl(k, S_h)][i] for k, cf in taps.items()) + (1 << 11)) >> 12
                t = scalar_blend(t, mm[cl(nr, S_h)][i], mm[cl(nr + 1, S_h)][i], ar)
                P[j][i] = min(max((t * (1 << u) + (1 << (n - 1))) >> n, 0), (1 << D) - 1)
        if c == 0:
            Q = [[0] * w for _ in range(h)]
            for j in range(h):
                for i in range(w):
                    win = [P[cl(j + dy, h)][cl(i + dx, w)] for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
                    ctr, e, f = win[4], win[1] + win[3] + win[5] + win[7], win[0] + win[2] + win[6] + win[8]
                    Q[j][i] = min(max(ctr + ((16 * ctr - (4 * ctr + 2 * e + f)) * g + 128 >> 8), min(win)), max(win))
            P = Q
        ch, cw = (SR.coded(dh), SR.coded(dw)) if c == 0 else (SR.coded(dh) // 2, SR.coded(dw) // 2)
        out.append(np.array([[P[min(j, h - 1)][min(i, w - 1)] for i in range(cw)] for j in range(ch)], R.out_dtype(D)))
    return out


@pytest.mark.parametrize("setting", SETTINGS, ids=SETTING_IDS)
@pytest.mark.parametrize("case,B,D", [(CASES[9], 8, 8), (CASES[9], 16, 10), (CASES[8], 10, 8), (CASES[7], 8, 10)], ids=lambda x: case_id(x) if isinstance(x, tuple) else str(x))
def test_model_equals_the_scalar_restatement(case, B, D, setting):
    diff = same_planes(model(case, B, D, setting), scalar_upscale(source(case, B), B, *case[1], D, *setting))
    assert not diff, diff


# ------------------------------------------------------------------------------------------------ 3. properties of the model
def test_model_keeps_a_constant_plane_at_the_rails_too():
    for (sw, sh), (dw, dh) in CASES:
        for B, D in ((8, 8), (10, 8), (16, 10), (8, 10)):
            for val in (0, 1, (1 << B) - 1):
                y = np.full((sh, sw), val, R.src_dtype(B))
                c = np.full((sh // 2, sw // 2), val, R.src_dtype(B))
                want = (val << (D - B)) if D >= B else min((val + (1 << (B - D - 1))) >> (B - D), (1 << D) - 1)
                for g, ar in SETTINGS:
                    for p in R.upscale(y, c, c, B, dw, dh, D, g, ar):
                        assert np.all(p == want), ((sw, sh), (dw, dh), B, D, val, g, ar)


@pytest.mark.parametrize("B,D", DEPTHS)
def test_model_with_full_antiring_stays_inside_the_source_range(B, D):
    for case in CASES:
        src = [np.minimum(p.astype(np.int64), (1 << B) - 1) for p in source(case, B)]
        for P, s in zip(R.interpolate(*source(case, B), B, *case[1], D, 8), src):
            lo, hi = int(s.min()), int(s.max())
            if D >= B:
                lo, hi = lo << (D - B), hi << (D - B)
            else:
                lo, hi = (lo + (1 << (B - D - 1))) >> (B - D), min((hi + (1 << (B - D - 1))) >> (B - D), (1 << D) - 1)
            assert lo <= int(P.min()) and int(P.max()) <= hi, (case_id(case), lo, hi, int(P.min()), int(P.max()))


def test_model_random_sources_overshoot_both_ways_without_antiring():
    """what the clamp has to do: the plain cubic leaves the source range on these sources, above and below"""
    P = R.interpolate(*source(CASES[2], 8), 8, *CASES[2][1], 8, 0)[0]
    Pc = R.interpolate(*source(CASES[2], 8), 8, *CASES[2][1], 8, 8)[0]
    assert (P > Pc).any() and (P < Pc).any()


@pytest.mark.parametrize("setting", SETTINGS, ids=SETTING_IDS)
def test_model_sharpened_luma_stays_inside_its_3x3(setting):
    g, ar = setting
    for case in CASES:
        for B, D in ((8, 8), (16, 10)):
            (dw, dh) = case[1]
            P = R.interpolate(*source(case, B), B, dw, dh, D, ar)
            out = model(case, B, D, setting)
            q = np.pad(P[0], 1, mode="edge")
            win = [q[dy:dy + dh, dx:dx + dw] for dy in range(3) for dx in range(3)]
            luma = out[0][:dh, :dw].astype(np.int64)
            assert np.all(luma >= np.minimum.reduce(win)) and np.all(luma <= np.maximum.reduce(win))
            if g == 0:
                assert np.array_equal(luma, P[0])
            assert np.array_equal(out[1][:dh // 2, :dw // 2], P[1]) and np.array_equal(out[2][:dh // 2, :dw // 2], P[2])      # chroma is P as it is


@pytest.mark.parametrize("B,D", [(b, d) for b in (8, 10, 12, 16) for d in (8, 10)])
def test_model_one_to_one_is_the_downscaler_at_one_to_one(B, D):
    for w, h in ((70, 38), (136, 72)):
        src = SR.random_source(w, h, B, w + B + D, full_word=True)
        want = SR.scale(*src, B, w, h, D)
        for ar in range(9):
            assert not same_planes(R.upscale(*src, B, w, h, D, 0, ar), want), ar


# ------------------------------------------------------------------------------------------------ 4. scale_taps.h against the model's tables
@pytest.fixture(scope="module")
def emu():
    lib = util.stepped_library()
    lib.emu_upscale.argtypes = [C.POINTER(_lib.UpscaleSrc)] + [C.c_void_p] * 3 + [C.c_int] * 5 + [C.c_uint] + [C.c_void_p] * 3 + [C.POINTER(C.c_int)]
    lib.emu_upscale_taps.argtypes = [C.c_int] * 3 + [C.c_void_p] * 3 + [C.POINTER(C.c_int)]
    lib.emu_upscale_block.argtypes = [C.c_int] * 4
    lib.emu_upscale_tile.argtypes = [C.POINTER(C.c_int)] * 4
    return lib


SIZE_PAIRS = CASES + [(s, (100, 70)) for s in SOURCES] + [((960, 540), (1920, 1080)), ((1280, 720), (1920, 1080)), ((1920, 1080), (3840, 2160)), ((640, 360), (1920, 1080)),
                                                          ((854, 480), (1920, 1080)), ((720, 576), (1350, 1080)), ((48, 40), (96, 80)), ((16, 16), (64, 64))]


def axis_pairs():
    pairs = {(1000, 1002), (16, 16), (16, 64), (998, 3991)}
    for (sw, sh), (dw, dh) in SIZE_PAIRS:
        pairs |= {(sw, dw), (sh, dh), (sw // 2, dw // 2), (sh // 2, dh // 2)}
    return sorted(pairs)


@pytest.mark.parametrize("p", [1, 2])
def test_header_tables_equal_the_model(emu, p):
    worst = (0, None)
    for S, Dn in axis_pairs():
        first, near, coef, taps = np.zeros(Dn, np.int32), np.zeros(Dn, np.int32), np.zeros((Dn, R.TAPS), np.int16), C.c_int()
        assert emu.emu_upscale_taps(S, Dn, p, first.ctypes.data, near.ctypes.data, coef.ctypes.data, C.byref(taps)) == 0, (S, Dn)
        want_first, want_near, want_coef, longest = R.table(S, Dn, p)
        assert np.array_equal(first, want_first) and np.array_equal(near, want_near) and np.array_equal(coef, want_coef) and taps.value == longest, (S, Dn)
        c = coef.astype(np.int64)
        mag = np.abs(c).sum(axis=1)
        assert np.all(c.sum(axis=1) == 4096) and mag.max() <= 5120 and longest <= 4, (S, Dn)
        assert np.all(np.diff(near) >= 0) and np.all(first >= near - 1) and np.all(first + (c != 0).cumsum(axis=1).argmax(axis=1) <= near + 2)
        assert S != Dn or longest == 1
        if mag.max() > worst[0]:
            worst = (int(mag.max()), (S, Dn, int(mag.argmax()), c[mag.argmax()].tolist()))
    print("the row with the largest sum |c|:", worst)
    assert worst[0] == 5120          # phase 1/2, [-256, 2304, 2304, -256]: reached (2:3 centre aligned: 48 -> 72) and never passed


def test_header_refuses_what_the_definition_excludes(emu):
    buf, taps = np.zeros(80 * 4, np.int32), C.c_int()
    for S, Dn, p in ((17, 16, 2), (16, 65, 2), (16, 32, 0), (16, 32, 3), (0, 0, 2)):
        assert emu.emu_upscale_taps(S, Dn, p, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, C.byref(taps)) == -3, (S, Dn, p)


def test_block_builder_accepts_the_sizes_of_the_reference_rule(emu):
    for (sw, sh), (dw, dh) in SIZE_PAIRS:
        assert emu.emu_upscale_block(sw, sh, dw, dh) == 0, ((sw, sh), (dw, dh))
    assert emu.emu_upscale_block(32, 32, 16, 16) == -3 and emu.emu_upscale_block(16, 16, 66, 64) == -3


# ------------------------------------------------------------------------------------------------ 5. the kernel program stepped on the CPU
def emu_upscale(emu, case, B, D, setting, order=0, align=16, seed=1):
    (sw, sh), (dw, dh) = case
    want = model(case, B, D, setting)
    out = [np.full(p.shape, 0x77, p.dtype) for p in want]
    stats = (C.c_int * 4)()
    rc = emu.emu_upscale(C.byref(_lib.UpscaleSrc(sw, sh, B, *setting)), *[p.ctypes.data for p in source(case, B)], dw, dh, D, order, align, seed,
                         *[p.ctypes.data for p in out], stats)
    assert rc == 0, rc
    assert stats[0] == 0, f"{stats[0]} misaligned accesses"
    assert stats[1] == 0, f"{stats[1]} samples written outside the coded width"
    assert (stats[2], stats[3]) == (align, align)
    return same_planes(out, want)


def test_sizes_meet_the_tile_edges(emu):
    tw, th, halo, rows = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    emu.emu_upscale_tile(C.byref(tw), C.byref(th), C.byref(halo), C.byref(rows))
    assert 136 > tw.value and 136 % tw.value and 72 > th.value and 72 % th.value          # 136x72: more than one tile each way, partial tiles
    assert R.coded(70) == 72 and R.coded(38) == 40 and (R.coded(70) // 2) % 8 == 4         # 70x38: margin on both sides, a chroma row that ends with half a run
    assert halo.value == 1 and rows.value >= th.value + 2 * halo.value + 3                 # 1:1: the near of the rows of a tile with its halo, and four around them


@pytest.mark.parametrize("B,D", DEPTHS)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_stepped_kernel_equals_model(emu, case, B, D):
    for k, setting in enumerate(SETTINGS):
        for order in (0, 1, 2):
            diff = emu_upscale(emu, case, B, D, setting, order, 16, seed=17 * order + B + k)
            assert not diff, (setting, order, diff)


@pytest.mark.parametrize("align", [1, 4, 8])
@pytest.mark.parametrize("B,D", DEPTHS)
def test_stepped_kernel_with_misaligned_planes(emu, B, D, align):
    """the same grid on planes of the narrower alignment classes: every case, depth pair and setting, the lane order turning with them"""
    for i, case in enumerate(CASES):
        for k, setting in enumerate(SETTINGS):
            diff = emu_upscale(emu, case, B, D, setting, (i + k) % 3, align, seed=align + 5 * k)
            assert not diff, (case, setting, diff)


def test_stepped_kernel_clamps_values_above_the_declared_depth():
    assert max(int(p.max()) for p in source(CASES[2], 10)) > 60000          # what every 10-bit case above was fed


def test_stepped_kernel_under_address_sanitizer(tmp_path):
    """a stand-alone program (its own main, no python in the process): the table builder and the stepped kernel over source planes allocated to end with their last
    sample, every ratio, element type, alignment class and setting.  A read past a plane ends it with the sanitizer's report"""
    exe = tmp_path / "upscale_asan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-w", "-o", str(exe),
                    str(ROOT / "tests" / "emu" / "upscale.cpp"), str(ROOT / "tests" / "upscale_asan_main.cc")], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert p.stdout.strip() == "288 runs"


# ------------------------------------------------------------------------------------------------ 6. the entry points without a device
def upscale_call(sw=64, sh=48, dw=128, dh=96, B=8, D=8, **over):
    src = R.random_source(sw, sh, B, 1)
    pw, ph = R.coded(dw), R.coded(dh)
    out = [np.zeros(s, R.out_dtype(D)) for s in ((ph, pw), (ph // 2, pw // 2), (ph // 2, pw // 2))]
    a = dict(src=_lib.UpscaleSrc(sw, sh, B, 8, 8), y=src[0].ctypes.data, u=src[1].ctypes.data, v=src[2].ctypes.data, pitch_y=sw, pitch_c=sw // 2, dw=dw, dh=dh, D=D,
             oy=out[0].ctypes.data, ou=out[1].ctypes.data, ov=out[2].ctypes.data)
    a.update(over)
    rc = _lib.load().mihevc_k_upscale_source(0, None if a["src"] is None else C.byref(a["src"]), a["y"], a["u"], a["v"], a["pitch_y"], a["pitch_c"], a["dw"], a["dh"], a["D"],
                                             a["oy"], a["ou"], a["ov"])
    del src, out
    return rc


def test_upscale_source_rejects_bad_arguments():
    assert upscale_call(src=None) == _lib.EINVAL
    for sw, sh, dw, dh in ((63, 48, 128, 96), (64, 47, 128, 96), (64, 48, 127, 96), (64, 48, 128, 95), (14, 48, 14, 96), (64, 14, 128, 14),      # odd, too small
                           (130, 48, 128, 96), (64, 98, 128, 96), (30, 48, 128, 96), (64, 22, 128, 96)):                                         # reducing, beyond 1:4
        assert upscale_call(sw, sh, dw, dh) == _lib.EINVAL, (sw, sh, dw, dh)
    for B in (7, 17, 0):
        assert upscale_call(src=_lib.UpscaleSrc(64, 48, B, 8, 8)) == _lib.EINVAL
    for g, ar in ((65, 8), (-1, 8), (8, 9), (8, -1)):
        assert upscale_call(src=_lib.UpscaleSrc(64, 48, 8, g, ar)) == _lib.EINVAL
    for i in range(3):
        src = _lib.UpscaleSrc(64, 48, 8, 8, 8)
        src.reserved[i] = 1
        assert upscale_call(src=src) == _lib.EINVAL
    assert upscale_call(pitch_y=63) == _lib.EINVAL and upscale_call(pitch_c=31) == _lib.EINVAL
    assert upscale_call(D=9) == _lib.EINVAL and upscale_call(D=12) == _lib.EINVAL
    for k in ("y", "u", "v", "oy", "ou", "ov"):
        assert upscale_call(**{k: None}) == _lib.EINVAL, k


def test_send_frame_upscaled_rejects_a_null_session():
    y = np.zeros((48, 64), np.uint8)
    assert _lib.load().mihevc_send_frame_upscaled(None, C.byref(_lib.UpscaleSrc(64, 48, 8, 8, 8)), y.ctypes.data, y.ctypes.data, y.ctypes.data, 64, 32, 0, 0) == _lib.EINVAL


@pytest.mark.skipif(_lib.load().mihevc_device_count() > 0, reason="a GPU is present")
def test_no_gpu_means_loud_failure():
    assert upscale_call() == _lib.ENODEV and upscale_call(B=10, D=10) == _lib.ENODEV
    assert upscale_call(src=None) == _lib.EINVAL          # the arguments are judged first


def test_upscale_src_layout_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mihevc.h"\nint main(void){printf("%zu %zu %zu %zu %zu\\n",'
                   "sizeof(mihevc_upscale_src),offsetof(mihevc_upscale_src,bit_depth),offsetof(mihevc_upscale_src,sharpen),offsetof(mihevc_upscale_src,antiring),"
                   "offsetof(mihevc_upscale_src,reserved));return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    U = _lib.UpscaleSrc
    assert got == [C.sizeof(U), U.bit_depth.offset, U.sharpen.offset, U.antiring.offset, U.reserved.offset] and got[0] == 32
    assert _lib.load().mihevc_abi_version() == 6
    assert {"mihevc_send_frame_upscaled", "mihevc_k_upscale_source"} <= set(_lib.EXPORTS)


# ------------------------------------------------------------------------------------------------ 7. upscale_target and encode_file(upscale=)
def test_upscale_target_matches_the_recorded_sizes():
    from hevc_amd.encoder import upscale_target
    cases = json.loads((ROOT / "tests" / "golden" / "upscale_targets.json").read_text())["cases"]
    assert len(cases) >= 8
    for c in cases:
        assert list(upscale_target(c["width"], c["height"], c["target_height"])) == c["target"], c
        assert c["target"][0] == c["ref_width"] & ~1
    assert upscale_target(854, 480) == (1920, 1080)          # 1921 in the reference's arithmetic


class StubEncoder:
    """stands where the session would: keeps what encode_file hands it"""
    made = []

    def __init__(self, cfg, device=0):
        self.cfg, self.calls = cfg, []
        StubEncoder.made.append(self)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass

    def send_upscaled(self, width, height, y, u, v, bit_depth=None, sharpen=8, antiring=8, pts=None, asynchronous=False):
        self.calls.append((width, height, y.shape, u.shape, v.shape, str(y.dtype), bit_depth, sharpen, antiring, pts))

    def packets_dts(self):
        while len(self.calls) > getattr(self, "out", 0):
            self.out = getattr(self, "out", 0) + 1
            yield b"\x00\x00\x00\x01\x26\x01" + bytes(8), self.out - 1, self.out == 1, self.out - 1

    def flush(self):
        pass

    def headers(self):
        cfg = self.cfg
        buf = (C.c_uint8 * 4096)()
        n = _lib.load().mihevc_write_parameter_sets(C.byref(cfg), buf, 4096)
        assert n > 0
        return bytes(buf[:n])


def test_encode_file_enlarging_asks_the_pipe_for_the_source_as_it_is(fake_ffmpeg, tmp_path, monkeypatch):
    from hevc_amd import encoder, mp4
    sw, sh, n = 64, 48, 3
    monkeypatch.setenv("FAKE_FRAMES", str(n))
    monkeypatch.setenv("FAKE_FB", str(sw * sh * 3 // 2 * 2))
    monkeypatch.setattr(encoder, "Encoder", StubEncoder)
    StubEncoder.made.clear()
    out = tmp_path / "o.mp4"
    assert encoder.encode_file(tmp_path / "a.mov", out, info("yuv420p10le", sw, sh, n), total_frames=n, upscale=(128, 96), sharpen=12, antiring=6) == 0
    argv = fake_ffmpeg.read_text().split("\n")[-2].split()
    assert argv[argv.index("-pix_fmt") + 1] == "yuv420p10le" and not {"-s", "-vf", "-filter:v"} & set(argv) and not any("scale" in a for a in argv)
    (enc,) = StubEncoder.made
    assert (enc.cfg.width, enc.cfg.height, enc.cfg.bit_depth) == (128, 96, 10)
    assert enc.calls == [(sw, sh, (sh, sw), (sh // 2, sw // 2), (sh // 2, sw // 2), "uint16", 10, 12, 6, i) for i in range(n)]
    data = out.read_bytes()
    start, end = 0, len(data)
    for name in ("moov", "trak", "tkhd"):
        _, start, end = [b for b in mp4.parse_boxes(data, start, end) if b[0] == name][0]
    assert (int.from_bytes(data[end - 8:end - 4], "big") >> 16, int.from_bytes(data[end - 4:end], "big") >> 16) == (128, 96)      # the track has the target size
    from hevc_amd.transcoder import calculate_apple_hevc_level
    assert enc.cfg.level_idc == int(round(float(calculate_apple_hevc_level(info("yuv420p10le", 128, 96, n))[0]) * 30))      # the level follows the target size
    # a height and 'auto' go through upscale_target: 64x48 to 144 lines is 192x144; 'auto' asks for 1080 lines, more than four times 48
    for up, want in ((144, (192, 144)), ("auto", None)):
        StubEncoder.made.clear()
        rc = encoder.encode_file(tmp_path / "a.mov", tmp_path / "h.mp4", info("yuv420p10le", sw, sh, n), total_frames=n, upscale=up)
        if want is None:
            assert rc == 1 and not StubEncoder.made
        else:
            assert rc == 0 and (StubEncoder.made[0].cfg.width, StubEncoder.made[0].cfg.height) == want and StubEncoder.made[0].calls[0][7:9] == (8, 8)
    # what is refused, each with 1 and before a session exists: a target smaller than the source, a ratio above 4, odd targets, bad settings, every combination
    StubEncoder.made.clear()
    src_info = info("yuv420p10le", sw, sh, n)
    for kw in (dict(upscale=(62, 48)), dict(upscale=(64, 46)), dict(upscale=(258, 96)), dict(upscale=(128, 194)), dict(upscale=(127, 96)), dict(upscale=(128, 95)),
               dict(upscale="big"), dict(upscale=(128,)), dict(upscale=0), dict(upscale=True), dict(upscale=(128, 96), sharpen=65), dict(upscale=(128, 96), antiring=9),
               dict(upscale=(128, 96), size=(32, 24)), dict(upscale=(128, 96), native_rgb=True), dict(upscale=(128, 96), deinterlace="frame"),
               dict(upscale=(128, 96), denoise=2), dict(upscale=(128, 96), lut="hdr-to-sdr"), dict(upscale=(128, 96), interpolate=2),
               dict(upscale=(128, 96), devices=[0, 1]), dict(upscale=(128, 96), devices=[0, 1], row_split=True)):
        assert encoder.encode_file(tmp_path / "a.mov", tmp_path / "no.mp4", src_info, total_frames=n, **kw) == 1, kw
        assert not StubEncoder.made, kw
    # another layout with upscale=: an error, not a silent conversion
    monkeypatch.setenv("FAKE_FB", str(sw * sh * 2 * 2))
    assert encoder.encode_file(tmp_path / "a.mov", tmp_path / "p.mp4", info("yuv422p10le", sw, sh, n), total_frames=n, upscale=(128, 96)) == 1
    assert not StubEncoder.made or not StubEncoder.made[0].calls
