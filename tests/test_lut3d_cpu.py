"""CPU: the colour table source (mihevc_set_lut3d / mihevc_send_frame_lut3d / mihevc_k_lut3d).  The numpy model of tests/lut3d_ref.py against a
pixel-by-pixel restatement in Python integers and hand-worked pixels; the identities of the definition; the kernel program of hevc_amd/csrc/kernels/lut3d.h stepped
on the CPU (tests/emu/lut3d.cpp) against the model, bit for bit; its division over the whole range; the sanitizer program; hevc_amd/lut3d.py (.cube files,
quantisation, the HDR -> SDR table); the new entry points without a device; the ABI struct; encode_file(lut=) in front of a stand-in ffmpeg."""
import ctypes as C
import math
import subprocess
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

from hevc_amd import _lib, lut3d
from tests import lut3d_ref as R
from tests import util
from tests.ingest_common import fake_ffmpeg, same_planes      # noqa: F401 (fake_ffmpeg: a fixture)
from tests.lut3d_common import CASES, KINDS, MATRICES, NS, SIZES, case_id, model, source, src_struct, table, vp
from tests.test_deint_cpu import StubEncoder

ROOT = Path(__file__).resolve().parents[1]
KRKB = {1: (2126, 722), 5: (2990, 1140), 6: (2990, 1140), 9: (2627, 593)}


# ------------------------------------------------------------------------------------------------ 1. the model against a scalar restatement
def rdiv(num, den):
    """floor(num / den + 1/2) for den > 0, Python integers"""
    return (2 * num + den) // (2 * den)


def scalar_lookup(L, N, v):
    """step 3 for one pixel, every index written out.  L[b][g][r][c]"""
    i, f = [], []
    for c in range(3):
        p = v[c] * (N - 1)
        ic = min(p // 65535, N - 2)
        i.append(ic)
        f.append(p - 65535 * ic)
    axes = sorted(range(3), key=lambda a: -f[a])                  # stable: ties keep r before g before b
    f1, f2, f3 = (f[a] for a in axes)
    pos = list(i)
    verts = [tuple(pos)]
    for a in axes:
        pos[a] += 1
        verts.append(tuple(pos))
    w = (65535 - f1, f1 - f2, f2 - f3, f3)
    return [(sum(wk * int(L[b][g][r][c]) for wk, (r, g, b) in zip(w, verts)) + 32767) // 65535 for c in range(3)]


def scalar_picture(planes, B, matrix, full, L, D, out_matrix, out_full):
    """steps 1 to 4 pixel by pixel in Python integers; display-size planes (lists of lists) out"""
    Yp, Cb, Cr = ([[min(int(x), (1 << B) - 1) for x in row] for row in p] for p in planes)
    H, W = len(Yp), len(Yp[0])
    N = len(L)
    kr, kb = KRKB[matrix]
    kg = 10000 - kr - kb
    den_y = (1 << B) - 1 if full else 219 << (B - 8)
    den_c = (1 << B) - 1 if full else 224 << (B - 8)
    nY = rdiv(65535 << 16, den_y)
    nRv = rdiv(2 * (10000 - kr) * (65535 << 16), 10000 * 8 * den_c)
    nGu = rdiv(-2 * kb * (10000 - kb) * (65535 << 16), kg * 10000 * 8 * den_c)
    nGv = rdiv(-2 * kr * (10000 - kr) * (65535 << 16), kg * 10000 * 8 * den_c)
    nBu = rdiv(2 * (10000 - kb) * (65535 << 16), 10000 * 8 * den_c)
    oY, oC = (0 if full else 16 << (B - 8)), 1 << (B - 1)

    def h(c, i, x):
        return 2 * c[i][x // 2] if x % 2 == 0 else c[i][x // 2] + c[i][min(x // 2 + 1, W // 2 - 1)]

    def c8(c, x, y):
        j = y // 2
        return 3 * h(c, j, x) + h(c, max(j - 1, 0) if y % 2 == 0 else min(j + 1, H // 2 - 1), x)

    okr, okb = KRKB[out_matrix]
    okg = 10000 - okr - okb
    S = 32 - D
    sy_n, sc_n, ooY = ((1 << D) - 1, (1 << D) - 1, 0) if out_full else (219 << (D - 8), 224 << (D - 8), 16 << (D - 8))
    rows = [([okr, okg, okb], 10000, sy_n), ([-okr, -okg, 10000 - okb], 2 * (10000 - okb), sc_n), ([10000 - okr, -okg, -okb], 2 * (10000 - okr), sc_n)]
    m = [[rdiv(x * sn << S, den * 65535) for x in num] for num, den, sn in rows]
    t = [[None] * W for _ in range(H)]
    for y in range(H):
        for x in range(W):
            yy, cb, cr = Yp[y][x] - oY, c8(Cb, x, y) - 8 * oC, c8(Cr, x, y) - 8 * oC
            v = [min(max((tt + (1 << 15)) >> 16, 0), 65535) for tt in (nY * yy + nRv * cr, nY * yy + nGu * cb + nGv * cr, nY * yy + nBu * cb)]
            o = scalar_lookup(L, N, v)
            t[y][x] = [sum(m[r][c] * o[c] for c in range(3)) for r in range(3)]
    peak = (1 << D) - 1
    out_y = [[min(max(((t[y][x][0] + (1 << (S - 1))) >> S) + ooY, 0), peak) for x in range(W)] for y in range(H)]
    out_c = []
    for c in (1, 2):
        out_c.append([[min(max(((sum(t[r][max(2 * i - 1, 0)][c] + 2 * t[r][2 * i][c] + t[r][2 * i + 1][c] for r in (2 * j, 2 * j + 1)) + (1 << (S + 2))) >> (S + 3))
                                + (1 << (D - 1)), 0), peak) for i in range(W // 2)] for j in range(H // 2)])
    return [out_y] + out_c


@pytest.mark.parametrize("B,D,matrix,full,out_matrix,out_full,n", [(8, 8, 1, 0, 9, 1, 2), (10, 8, 9, 0, 1, 0, 3), (12, 10, 5, 1, 6, 0, 5), (10, 10, 6, 1, 1, 1, 4)])
def test_model_equals_the_definition_pixel_by_pixel(B, D, matrix, full, out_matrix, out_full, n):
    """tiny pictures of noise (above 8 bit with values above the depth): every pixel, every clamp of steps 1 and 4 at the four edges"""
    W, H = 10, 6
    src = R.source("noise", W, H, B, seed=n)
    L = R.random_table(n, n)
    got = R.convert(src, B, matrix, full, L, D, out_matrix, out_full)
    want = scalar_picture(src, B, matrix, full, L.tolist(), D, out_matrix, out_full)
    for g, w_, (hh, ww) in zip(got, want, ((H, W), (H // 2, W // 2), (H // 2, W // 2))):
        assert np.array_equal(g[:hh, :ww], np.array(w_)), (B, D, matrix)
    assert got[0].shape == (8, 16) and np.all(got[0][:, W:] == got[0][:, W - 1:W]) and np.all(got[1][H // 2:] == got[1][H // 2 - 1:H // 2])


def test_coefficients_by_hand():
    """BT.709 limited at 8 bit: sY = 65535 / 219, sC = 65535 / 224.  The integers are worked out here from the ratios and compared with the decimal values of the
    coefficients; nothing is taken from the code under test"""
    ny, nrv, ngu, ngv, nbu = R.inverse_coefficients(1, 0, 8)
    assert ny == (2 * 65535 * 65536 + 219) // (2 * 219)
    assert nrv == math.floor(Fraction(2 * 7874 * 65535 * 65536, 10000 * 224 * 8) + Fraction(1, 2))
    assert abs(nrv / 65536 - 2 * 0.7874 * 65535 / 224 / 8) < 1e-4 and abs(nbu / 65536 - 2 * 0.9278 * 65535 / 224 / 8) < 1e-4
    assert abs(ngu / 65536 + 2 * 0.0722 * 0.9278 / 0.7152 * 65535 / 224 / 8) < 1e-4 and abs(ngv / 65536 + 2 * 0.2126 * 0.7874 / 0.7152 * 65535 / 224 / 8) < 1e-4
    assert R.inverse_coefficients(9, 1, 12)[0] == (2 * 65535 * 65536 + 4095) // (2 * 4095)


# the six orderings of the three fractions on a one-cell table (N = 2: i = 0 and f = v): the path V0 -> V1 -> V2 -> V3 through the cube's corners (r, g, b)
ORDERINGS = [((50000, 30000, 10000), [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1)]),      # r >= g >= b
             ((50000, 10000, 30000), [(0, 0, 0), (1, 0, 0), (1, 0, 1), (1, 1, 1)]),      # r >= b >= g
             ((30000, 50000, 10000), [(0, 0, 0), (0, 1, 0), (1, 1, 0), (1, 1, 1)]),      # g >= r >= b
             ((10000, 50000, 30000), [(0, 0, 0), (0, 1, 0), (0, 1, 1), (1, 1, 1)]),      # g >= b >= r
             ((30000, 10000, 50000), [(0, 0, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1)]),      # b >= r >= g
             ((10000, 30000, 50000), [(0, 0, 0), (0, 0, 1), (0, 1, 1), (1, 1, 1)])]      # b >= g >= r


@pytest.mark.parametrize("v,path", ORDERINGS)
def test_model_one_pixel_per_ordering_by_hand(v, path):
    L = R.random_table(2, 1)
    f1, f2, f3 = sorted(v, reverse=True)
    assert (f1, f2, f3) == (50000, 30000, 10000)
    w = (15535, 20000, 20000, 10000)
    want = [(sum(wk * int(L[b, g, r, c]) for wk, (r, g, b) in zip(w, path)) + 32767) // 65535 for c in range(3)]
    got = R.lookup(L, [np.array([x]) for x in v])
    assert [int(g[0]) for g in got] == want == scalar_lookup(L.tolist(), 2, list(v))


def test_model_ties_grid_points_and_the_last_cell():
    L = R.random_table(2, 2)
    # ties: the vertices the two orders disagree on have weight 0.  r = g > b: V1 is (1,0,0) or (0,1,0) with weight f1 - f2 = 0
    for v, terms in (((40000, 40000, 10000), [(25535, (0, 0, 0)), (30000, (1, 1, 0)), (10000, (1, 1, 1))]),
                     ((40000, 10000, 10000), [(25535, (0, 0, 0)), (30000, (1, 0, 0)), (10000, (1, 1, 1))]),
                     ((12345, 12345, 12345), [(53190, (0, 0, 0)), (12345, (1, 1, 1))])):
        want = [(sum(wk * int(L[b, g, r, c]) for wk, (r, g, b) in terms) + 32767) // 65535 for c in range(3)]
        assert [int(g[0]) for g in R.lookup(L, [np.array([x]) for x in v])] == want
    # f = 0 on every axis: exactly a grid point, N = 4 (65535 / 3 = 21845)
    L4 = R.random_table(4, 3)
    got = R.lookup(L4, [np.array([21845]), np.array([43690]), np.array([0])])
    assert [int(g[0]) for g in got] == [int(x) for x in L4[0, 2, 1]]
    # v = 65535: the last cell, i = N - 2 with f = 65535: the last grid point
    for n in (2, 4, 17, 65):
        Ln = R.random_table(n, n)
        got = R.lookup(Ln, [np.array([65535]), np.array([0]), np.array([65535])])
        assert [int(g[0]) for g in got] == [int(x) for x in Ln[n - 1, 0, n - 1]]
    # N = 2 is one cell: the corners come back
    for r, g, b in ((0, 0, 0), (1, 0, 1), (1, 1, 1), (0, 1, 0)):
        got = R.lookup(L, [np.array([65535 * r]), np.array([65535 * g]), np.array([65535 * b])])
        assert [int(x[0]) for x in got] == [int(x) for x in L[b, g, r]]


# ------------------------------------------------------------------------------------------------ 2. identity properties
@pytest.mark.parametrize("n", [2, 4, 6, 16])
def test_identity_table_returns_every_value(n):
    assert 65535 % (n - 1) == 0
    t = R.identity_table(n)
    assert np.array_equal(t, lut3d.identity(n))
    rng = np.random.default_rng(n)
    v = [np.concatenate([rng.integers(0, 65536, 20000), np.array([0, 1, 65534, 65535]), np.arange(n) * (65535 // (n - 1))]) for _ in range(3)]
    rng.shuffle(v[1])
    assert all(np.array_equal(o, x) for o, x in zip(R.lookup(t, v), v))


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("full", [0, 1])
@pytest.mark.parametrize("matrix", [1, 6, 9])
def test_flat_pictures_round_trip_under_the_identity(matrix, full, depth):
    """a flat picture under the identity table with the same matrix, range and depth on both sides: every colour whose R'G'B' needs no clipping (selected by step 2
    of the model, not from a list) comes back sample for sample.  Checked colour by colour on 200,000 random triples (a flat picture's step 1 gives 8 c and its
    step 4 filter 8 t), and on whole pictures through the model for a few of them"""
    rng = np.random.default_rng(10 * matrix + depth + full)
    peak = (1 << depth) - 1
    Y, cb, cr = (rng.integers(0, peak + 1, 200000) for _ in range(3))
    ok = R.in_gamut(Y, cb, cr, matrix, full, depth)
    assert 0.10 < ok.mean() < 0.30
    o = R.lookup(R.identity_table(16), R.to_rgb16(Y, 8 * cb, 8 * cr, matrix, full, depth))
    m, S, oy, oc = R.forward_coefficients(matrix, full, depth)
    t = [m[r][0] * o[0] + m[r][1] * o[1] + m[r][2] * o[2] for r in range(3)]
    y2 = np.clip(((t[0] + (1 << (S - 1))) >> S) + oy, 0, peak)
    c2 = [np.clip(((8 * x + (1 << (S + 2))) >> (S + 3)) + oc, 0, peak) for x in t[1:]]
    bad = ((y2 != Y) | (c2[0] != cb) | (c2[1] != cr)) & ok
    assert not bad.any(), int(bad.sum())
    for k in np.nonzero(ok)[0][:5]:
        flat = [np.full((16, 16), Y[k], R.dtype(depth)), np.full((8, 8), cb[k], R.dtype(depth)), np.full((8, 8), cr[k], R.dtype(depth))]
        assert not same_planes(R.convert(flat, depth, matrix, full, R.identity_table(16), depth, matrix, full), flat)


# ------------------------------------------------------------------------------------------------ 3. the kernel program stepped on the CPU
@pytest.fixture(scope="module")
def emu():
    lib = util.stepped_library()
    lib.emu_lut3d.argtypes = [C.POINTER(_lib.Lut3dSrc), C.c_int] + [C.c_void_p] * 4 + [C.c_int] * 7 + [C.c_void_p] * 3 + [C.POINTER(C.c_int)]
    lib.emu_lut3d_tile.argtypes = [C.POINTER(C.c_int)] * 2
    lib.emu_lut3d_inverse.argtypes = [C.c_int] * 3 + [C.POINTER(C.c_int)]
    lib.emu_lut3d_pixel.argtypes = [C.POINTER(_lib.Lut3dSrc), C.c_int, C.c_void_p] + [C.c_int] * 3 + [C.POINTER(C.c_int)] * 2
    return lib


def emu_lut3d(emu, case, order=0, align=16):
    c = case
    want = model(c)
    out = [np.full(p.shape, 0x77, p.dtype) for p in want]
    stats = (C.c_int * 4)()
    src = source(c.size, c.B, c.kind, c.n)
    rc = emu.emu_lut3d(C.byref(src_struct(c.B, c.matrix, c.full)), c.n, vp(table(c.n)), *[vp(p) for p in src], c.size[0], c.size[1], c.D, c.out_matrix, c.out_full,
                       order, align, *[vp(p) for p in out], stats)
    assert rc == 0, rc
    assert stats[0] == 0, f"{stats[0]} misaligned accesses"
    assert stats[1] == 0, f"{stats[1]} samples written outside the coded width"
    assert (stats[2], stats[3]) == (align, align)
    return same_planes(out, want)


def test_cases_cover_the_definition(emu):
    tw, th = C.c_int(), C.c_int()
    emu.emu_lut3d_tile(C.byref(tw), C.byref(th))
    assert 2 * tw.value < 520 < 3 * tw.value and 2 * th.value < 72 < 3 * th.value          # 520x72: two full tiles and a partial one each way
    assert 20 < th.value and 16 < th.value and 136 < tw.value                               # 136x20 and 16x16: fewer rows than a tile
    assert R.coded(70) == 72 and R.coded(36) == 40 and R.coded(70) % 16 == 8                # 70x36: margin on both axes, a row that ends with half a block
    assert {c.n for c in CASES if c.kind == "noise"} == set(NS) and {c.kind for c in CASES} == set(KINDS)
    for size in SIZES:
        assert {c.n for c in CASES if c.size == size} == set(NS)
    assert {(c.B, c.D) for c in CASES} == {(b, d) for b in (8, 10, 12) for d in (8, 10)}
    assert {c.matrix for c in CASES} == {c.out_matrix for c in CASES} == set(MATRICES)
    assert {(c.full, c.out_full) for c in CASES} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    for n in NS:
        assert table(n).min() == 0 and table(n).max() == 65535
    # the inputs: noise above the depth; a ramp whose fractions are all equal; samples on both sides of cell boundaries
    assert max(int(p.max()) for p in source((70, 36), 10, "noise", 33)) > 60000
    y, cb, cr = source((70, 36), 10, "ramp", 33)
    rgb = R.to_rgb16(y.astype(np.int64), R.chroma_to_luma_grid(cb), R.chroma_to_luma_grid(cr), 1, 0, 10)
    assert np.array_equal(rgb[0], rgb[1]) and np.array_equal(rgb[1], rgb[2])
    y, cb, cr = source((70, 36), 10, "cells", 33)
    r = R.to_rgb16(y.astype(np.int64), R.chroma_to_luma_grid(cb), R.chroma_to_luma_grid(cr), 1, 0, 10)[0]
    cell = r * 32 // 65535
    assert len(np.unique(cell)) >= 32 and ((r * 32 % 65535) < 64).any() and ((r * 32 % 65535) > 65535 - 64).any()


def test_stepped_coefficients_equal_the_model(emu):
    got = (C.c_int * 5)()
    for matrix in MATRICES:
        for full in (0, 1):
            for B in (8, 10, 12):
                assert emu.emu_lut3d_inverse(matrix, full, B, got) == 0
                assert tuple(got) == R.inverse_coefficients(matrix, full, B), (matrix, full, B)
    assert emu.emu_lut3d_inverse(2, 0, 8, got) == -3


@pytest.mark.parametrize("v,path", ORDERINGS)
def test_stepped_pixel_function_on_the_hand_worked_pixels(emu, v, path):
    """the kernel's pixel function alone, fed the Y'CbCr whose step 2 the model gives, on the one-cell table of the hand-worked pixels and on ties"""
    L = R.random_table(2, 1)
    rgb, out = (C.c_int * 3)(), (C.c_int * 3)()
    rng = np.random.default_rng(sum(v))
    for _ in range(200):
        Y, cb8, cr8 = int(rng.integers(0, 1024)), int(rng.integers(0, 8184)), int(rng.integers(0, 8184))
        assert emu.emu_lut3d_pixel(C.byref(src_struct(10, 9, 0)), 2, vp(L), Y, cb8, cr8, rgb, out) == 0
        want = R.to_rgb16(np.array([Y]), np.array([cb8]), np.array([cr8]), 9, 0, 10)
        assert list(rgb) == [int(x[0]) for x in want]
        assert list(out) == [int(x[0]) for x in R.lookup(L, want)] == scalar_lookup(L.tolist(), 2, list(rgb))
    # a grey (all fractions equal) and a pixel with chroma at its midpoint on one axis only
    for Y, cb8, cr8 in ((500, 4096, 4096), (64, 4096, 4096), (940, 4096, 4096), (700, 4096, 5000)):
        assert emu.emu_lut3d_pixel(C.byref(src_struct(10, 9, 0)), 2, vp(L), Y, cb8, cr8, rgb, out) == 0
        assert list(out) == scalar_lookup(L.tolist(), 2, list(rgb))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_stepped_kernel_equals_model(emu, case):
    for order in (0, 1, 2):
        diff = emu_lut3d(emu, case, order)
        assert not diff, (order, diff)


@pytest.mark.parametrize("align", [1, 4, 8])
def test_stepped_kernel_with_misaligned_planes(emu, align):
    for i, case in enumerate(CASES):
        if case.kind == "noise":
            diff = emu_lut3d(emu, case, i % 3, align)
            assert not diff, (case, diff)


def test_stepped_division_is_exact_over_the_whole_range(emu):
    """(x + 1 + (x >> 16)) >> 16 against integer division by 65535: both ends of every quotient's dividends up to 65535 x 65536, the blend's largest dividend, and
    every p up to 65535 x 64"""
    assert emu.emu_lut3d_div_check() == 0


def test_stepped_kernel_under_address_sanitizer(tmp_path):
    """a stand-alone program (its own main, no python in the process): the stepped kernel over source planes and a table allocated to end with their last element,
    every size, source depth, output depth and alignment class.  A read past a plane or the table ends it with the sanitizer's report"""
    exe = tmp_path / "lut3d_asan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-w", "-o", str(exe),
                    str(ROOT / "tests" / "emu" / "lut3d.cpp"), str(ROOT / "tests" / "lut3d_asan_main.cc")], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert p.stdout.strip() == "96 runs"


# ------------------------------------------------------------------------------------------------ 4. hevc_amd/lut3d.py
def test_cube_round_trip(tmp_path):
    t = R.random_table(5, 4)
    lut3d.write_cube(tmp_path / "a.cube", t, title="five points")
    text = (tmp_path / "a.cube").read_text()
    assert text.startswith('TITLE "five points"\nLUT_3D_SIZE 5\nDOMAIN_MIN 0 0 0\nDOMAIN_MAX 1 1 1\n')
    back = lut3d.read_cube(tmp_path / "a.cube")
    assert back.shape == (5, 5, 5, 3) and back.dtype == np.float64 and np.array_equal(lut3d.quantise(back), t)
    # red varies fastest: the second entry of the file is L[0][0][1]
    assert np.array_equal(lut3d.quantise(np.array([float(x) for x in text.split("\n")[5].split()])), t[0, 0, 1])
    # floats round trip exactly; comments, blank lines and a title are skipped
    f = np.random.default_rng(1).random((3, 3, 3, 3))
    lut3d.write_cube(tmp_path / "f.cube", f)
    assert np.array_equal(lut3d.read_cube(tmp_path / "f.cube"), f)
    body = "\n".join(" ".join(repr(float(x)) for x in e) for e in f.reshape(-1, 3))
    (tmp_path / "c.cube").write_text(f"# made by hand\n\nTITLE \"t\"\n  LUT_3D_SIZE 3\n# no domain lines\n{body}\n\n")
    assert np.array_equal(lut3d.read_cube(tmp_path / "c.cube"), f)


def test_read_cube_refusals(tmp_path):
    body2 = "0 0 0\n" * 8

    def refused(text, what):
        (tmp_path / "x.cube").write_text(text)
        with pytest.raises(ValueError, match=what):
            lut3d.read_cube(tmp_path / "x.cube")
    refused("LUT_3D_SIZE 2\nDOMAIN_MIN 0 0 0\nDOMAIN_MAX 2 2 2\n" + body2, "domain")
    refused("LUT_3D_SIZE 2\nDOMAIN_MIN -1 0 0\n" + body2, "domain")
    refused("LUT_1D_SIZE 8\n" + "0 0 0\n" * 8, "1D")
    refused("LUT_3D_SIZE 2\n" + "0 0 0\n" * 7, "7 entries")
    refused("LUT_3D_SIZE 2\n" + "0 0 0\n" * 9, "9 entries")
    refused("LUT_3D_SIZE 1\n0 0 0\n", "outside")
    refused("LUT_3D_SIZE 66\n", "outside")
    refused("LUT_3D_SIZE 2\n" + "0 0 0\n" * 7 + "0 nan 0\n", "finite")
    refused("LUT_3D_SIZE 2\n" + "0 0 0\n" * 7 + "0 inf 0\n", "finite")
    refused("LUT_3D_SIZE 2\n" + "0 0 0\n" * 7 + "0 0\n", "three values")
    refused("LUT_3D_SIZE 2\n" + "0 0 0\n" * 7 + "0 0 x\n", "malformed")
    refused(body2, "LUT_3D_SIZE")
    refused("LUT_3D_SIZE 2\nLUT_3D_INPUT_RANGE 0 1\n" + body2, "unknown keyword")
    for bad in (1, 66, 2.0, True, None):
        with pytest.raises(ValueError):
            lut3d.identity(bad)
    with pytest.raises(ValueError):
        lut3d.as_uint16(np.zeros((2, 2, 3, 3)))
    with pytest.raises(ValueError):
        lut3d.as_uint16(np.full((2, 2, 2, 3), 70000, np.int64))
    with pytest.raises(ValueError):
        lut3d.quantise(np.array([0.0, np.nan]))


def test_quantise():
    """rint in float64 after the clip: ties go to the even neighbour (k + 1/2 is exact in the product for these), values outside [0, 1] are clipped"""
    x = np.array([0.5, 1.5, 2.5, 32767.5]) / 65535.0
    assert np.array_equal(x * 65535.0, [0.5, 1.5, 2.5, 32767.5])
    assert lut3d.quantise(x).tolist() == [0, 2, 2, 32768]
    assert lut3d.quantise(np.array([-0.1, 0.0, 1.0, 1.5, 0.49 / 65535, 0.51 / 65535])).tolist() == [0, 0, 65535, 65535, 0, 1]
    assert lut3d.quantise(np.array([0.25])).dtype == np.uint16
    assert np.array_equal(lut3d.as_uint16(np.full((2, 2, 2, 3), 0.5)), np.full((2, 2, 2, 3), 32768, np.uint16))      # 32767.5: to the even neighbour


@pytest.mark.parametrize("transfer", ["pq", "hlg"])
@pytest.mark.parametrize("peak", [1000.0, 4000.0])
def test_hdr_to_sdr_properties(transfer, peak):
    n = 33
    t = lut3d.hdr_to_sdr(n, transfer, peak)
    assert t.shape == (n, n, n, 3) and t.dtype == np.uint16
    assert t[0, 0, 0].tolist() == [0, 0, 0]                                                   # black stays black
    grey = np.array([t[k, k, k] for k in range(n)], np.int64)
    assert (grey.max(axis=1) - grey.min(axis=1)).max() <= 1                                   # the grey axis stays neutral
    assert np.all(np.diff(grey, axis=0) >= 0)                                                 # and does not fall
    # input at or above the peak maps to 65535 on the grey axis (PQ: the code value of peak_nits; HLG: code value 1 is the display's peak)
    at_peak = float(lut3d.pq_inverse_eotf(peak)) if transfer == "pq" else 1.0
    for e in (at_peak, min(at_peak * 1.05, 1.0), 1.0):
        assert lut3d.quantise(lut3d.hdr_to_sdr_function(np.full(3, e), transfer, peak)).tolist() == [65535] * 3
    assert all(t[k, k, k].tolist() == [65535] * 3 for k in range(n) if k / (n - 1) >= at_peak)
    # the table is the float64 function at every grid point, to rint
    ax = np.arange(n) / (n - 1)
    b, g, r = np.meshgrid(ax, ax, ax, indexing="ij")
    assert np.array_equal(t, np.rint(lut3d.hdr_to_sdr_function(np.stack([r, g, b], axis=-1), transfer, peak) * 65535).astype(np.uint16))
    # a fine grey ramp through the function itself: neutral, monotone, 0 at 0
    e = np.linspace(0, 1, 4001)
    f = lut3d.hdr_to_sdr_function(np.stack([e, e, e], axis=-1), transfer, peak)
    assert np.all(np.diff(f[:, 0]) >= 0) and np.abs(f - f[:, :1]).max() * 65535 < 0.5 and f[0].tolist() == [0, 0, 0]


def test_hdr_to_sdr_arguments():
    for kw in (dict(transfer="sdr"), dict(peak_nits=50.0), dict(peak_nits=float("nan")), dict(n=1), dict(n=66)):
        with pytest.raises(ValueError):
            lut3d.hdr_to_sdr(**{"n": 5, **kw})
    assert abs(float(lut3d.pq_eotf(lut3d.pq_inverse_eotf(203.0))) - 203.0) < 1e-9 and abs(float(lut3d.pq_eotf(0.508078)) - 100.0) < 0.05
    assert np.abs(lut3d.BT2020_TO_BT709.sum(axis=1) - 1).max() < 1e-12 and abs(lut3d.BT2020_TO_BT709[0, 0] - 1.6605) < 1e-4


def test_hdr_to_sdr_fidelity_of_65_points():
    """hdr_to_sdr(65) through step 3 of the model on 200,000 uniformly random PQ pixels against the float64 function evaluated at those pixels (the reference is the
    direct evaluation, not the table), in 8-bit output codes.  The largest differences sit where the 2020 -> 709 clip sets in (a component that the function
    clips to 0 while a neighbouring grid point has it above 0; the inverse gamma is steepest there), not on the neutral axis or inside the BT.709 gamut's bulk"""
    rng = np.random.default_rng(65)
    v = rng.integers(0, 65536, (200000, 3))
    looked = np.stack(R.lookup(lut3d.hdr_to_sdr(65), [v[:, 0], v[:, 1], v[:, 2]]), axis=1) / 65535.0 * 255.0
    d = np.abs(looked - lut3d.hdr_to_sdr_function(v / 65535.0) * 255.0)
    print(f"65 points, PQ, 1000 cd/m2: maximum {d.max():.2f}, mean {d.mean():.3f} 8-bit codes; {100 * (d.max(axis=1) > 1).mean():.1f} % of the pixels above 1 code")
    assert d.max() <= 76          # recorded 2026-10-19: maximum 37.97, mean 0.135; the bound is twice the recorded maximum, rounded up
    assert d.mean() <= 0.27       # likewise


# ------------------------------------------------------------------------------------------------ 5. the entry points without a device
def k_call(w=64, h=48, B=10, D=8, n=5, **over):
    src = R.source("noise", w, h, B)
    pw, ph = R.coded(w), R.coded(h)
    out = [np.zeros(s, R.dtype(D)) for s in ((ph, pw), (ph // 2, pw // 2), (ph // 2, pw // 2))]
    tab = R.random_table(n if 2 <= n <= 65 else 2, 1)          # (kept alive until the call has returned, as src and out are)
    a = dict(src=src_struct(B, 9, 0), n=n, table=vp(tab), y=vp(src[0]), u=vp(src[1]), v=vp(src[2]), pitch_y=w, pitch_c=w // 2, w=w, h=h, D=D, om=1, of=0,
             out=(C.c_void_p * 3)(*[p.ctypes.data for p in out]), stride=(C.c_int * 3)(pw, pw // 2, pw // 2))
    a.update(over)
    rc = _lib.load().mihevc_k_lut3d(0, None if a["src"] is None else C.byref(a["src"]), a["n"], a["table"], a["y"], a["u"], a["v"], a["pitch_y"], a["pitch_c"],
                                    a["w"], a["h"], a["D"], a["om"], a["of"], a["out"], a["stride"])
    del src, out, tab
    return rc


def test_k_lut3d_rejects_bad_arguments():
    for w, h in ((63, 48), (64, 47), (14, 48), (64, 14)):
        assert k_call(w=w, h=h, pitch_y=64, pitch_c=32) == _lib.EINVAL, (w, h)
    assert k_call(pitch_y=63) == _lib.EINVAL and k_call(pitch_c=31) == _lib.EINVAL
    for n in (1, 66, 0, -3):
        assert k_call(n=n) == _lib.EINVAL
    for B in (9, 14, 16, 0):
        assert k_call(src=_lib.Lut3dSrc(B, 9, 0)) == _lib.EINVAL
    for m in (0, 2, 4, 7, 10):
        assert k_call(src=_lib.Lut3dSrc(10, m, 0)) == _lib.EINVAL and k_call(om=m) == _lib.EINVAL
    assert k_call(src=_lib.Lut3dSrc(10, 9, 2)) == _lib.EINVAL and k_call(of=2) == _lib.EINVAL and k_call(D=9) == _lib.EINVAL and k_call(D=12) == _lib.EINVAL
    for k in range(4):
        s = _lib.Lut3dSrc(10, 9, 0)
        s.reserved[k] = 1
        assert k_call(src=s) == _lib.EINVAL
    for k in ("src", "table", "y", "u", "v", "out", "stride"):
        assert k_call(**{k: None}) == _lib.EINVAL, k
    z = np.zeros((48, 64), np.uint16)
    assert k_call(y=C.c_void_p(z.ctypes.data + 1)) == _lib.EINVAL                                 # a plane misaligned to its element
    assert k_call(out=(C.c_void_p * 3)(z.ctypes.data, None, z.ctypes.data)) == _lib.EINVAL
    assert k_call(stride=(C.c_int * 3)(63, 32, 32)) == _lib.EINVAL


def test_session_entries_reject_a_null_session():
    y = np.zeros((48, 64), np.uint8)
    lib = _lib.load()
    assert lib.mihevc_send_frame_lut3d(None, C.byref(_lib.Lut3dSrc(8, 1, 0)), y.ctypes.data, y.ctypes.data, y.ctypes.data, 64, 32, 0, 0) == _lib.EINVAL
    t = R.random_table(2, 1)
    assert lib.mihevc_set_lut3d(None, 2, vp(t)) == _lib.EINVAL


@pytest.mark.skipif(_lib.load().mihevc_device_count() > 0, reason="a GPU is present")
def test_no_gpu_means_loud_failure():
    assert k_call() == _lib.ENODEV and k_call(B=8, D=10, h=50) == _lib.ENODEV
    assert k_call(n=66) == _lib.EINVAL          # the arguments are judged first


def test_lut3d_layout_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mihevc.h"\nint main(void){printf("%zu %zu %zu %zu %zu\\n",'
                   "sizeof(mihevc_lut3d_src),offsetof(mihevc_lut3d_src,bit_depth),offsetof(mihevc_lut3d_src,matrix),"
                   "offsetof(mihevc_lut3d_src,full_range),offsetof(mihevc_lut3d_src,reserved));return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    S = _lib.Lut3dSrc
    assert got == [C.sizeof(S), S.bit_depth.offset, S.matrix.offset, S.full_range.offset, S.reserved.offset] and got == [28, 0, 4, 8, 12]
    assert _lib.load().mihevc_abi_version() == 6
    assert {"mihevc_set_lut3d", "mihevc_send_frame_lut3d", "mihevc_k_lut3d"} <= set(_lib.EXPORTS)


# ------------------------------------------------------------------------------------------------ 6. encode_file(lut=)
class LutStub(StubEncoder):
    def set_lut3d(self, t):
        self.calls.append(("table", t.shape, str(t.dtype), int(t[-1, -1, -1, 0])))

    def send_lut3d(self, y, u, v, bit_depth, matrix, full_range=False, pts=None, asynchronous=False):
        self.calls.append(("lut3d", y.shape, u.shape, str(y.dtype), bit_depth, matrix, bool(full_range), pts))
        self.sent += 1


def test_encode_file_lut_in_front_of_the_pipe(fake_ffmpeg, tmp_path, monkeypatch):
    from hevc_amd import encoder, probe, transcoder
    w, h, n = 64, 48, 3
    monkeypatch.setenv("FAKE_FRAMES", str(n))
    monkeypatch.setenv("FAKE_FB", str(w * h * 3))          # 10-bit frames
    monkeypatch.setattr(encoder, "Encoder", LutStub)
    md = "G(13250,34500)B(7500,3000)R(34000,16000)WP(15635,16450)L(40000000,50)"
    hdr = probe.VideoInfo(w, h, 30.0, "bt2020", "smpte2084", "bt2020nc", "yuv420p10le", md, "1000,400", 0, True, "eng", n, n / 30.0)

    def run(out, info=hdr, **kw):
        StubEncoder.made.clear()
        rc = encoder.encode_file(tmp_path / "a.mov", tmp_path / out, info, total_frames=n, **kw)
        return rc, (StubEncoder.made[0] if StubEncoder.made else None)

    # the built-in table: PQ from the probe, 4000 nits from master_display; an 8-bit SDR session; the pipe keeps delivering the source's own 10-bit frames
    rc, enc = run("a.mp4", lut="hdr-to-sdr")
    argv = fake_ffmpeg.read_text().split("\n")[-2].split()
    assert rc == 0 and argv[argv.index("-pix_fmt") + 1] == "yuv420p10le" and not {"-vf", "-filter:v"} & set(argv)
    assert enc.calls[0] == ("table", (65, 65, 65, 3), "uint16", 65535)
    assert enc.calls[1:] == [("lut3d", (h, w), (h // 2, w // 2), "uint16", 10, 9, False, i) for i in range(n)]
    c = enc.cfg
    assert (c.bit_depth, c.colour_primaries, c.transfer, c.matrix, c.hdr10) == (8, 1, 1, 1, 0)
    sdr = probe.VideoInfo(w, h, 30.0, "bt709", "bt709", "bt709", "yuv420p", "", "", 0, False, "eng", n, n / 30.0)
    crf, _cq, maxrate, bufsize, gop = transcoder.calculate_dynamic_values(sdr)
    want = encoder.config_for(sdr, crf, maxrate, bufsize, gop, *transcoder.calculate_apple_hevc_level(sdr))
    assert bytes(c) == bytes(want)                                                                   # the session of an SDR clip, field for field
    assert hdr.hdr and hdr.color_transfer == "smpte2084"                                             # the caller's info is not touched
    # Main10 on request; a table of one's own; a .cube file
    rc, enc = run("b.mp4", lut="hdr-to-sdr", lut_bit_depth=10)
    assert rc == 0 and (enc.cfg.bit_depth, enc.cfg.hdr10, enc.cfg.transfer) == (10, 0, 1)
    rc, enc = run("c.mp4", lut=R.random_table(5, 1))
    assert rc == 0 and enc.calls[0] == ("table", (5, 5, 5, 3), "uint16", 65535) and len(enc.calls) == 1 + n
    lut3d.write_cube(tmp_path / "g.cube", lut3d.identity(4))
    rc, enc = run("d.mp4", lut=str(tmp_path / "g.cube"))
    assert rc == 0 and enc.calls[0] == ("table", (4, 4, 4, 3), "uint16", 65535)
    # without lut= nothing changes: an HDR10 session
    rc, enc = run("e.mp4")
    assert rc == 0 and enc.cfg.hdr10 == 1 and enc.cfg.bit_depth == 10 and enc.calls == [("plain", (h, w), i) for i in range(n)]
    # refused: together with the other sources, several devices, a depth other than 8 / 10, a file that is no table, a table of the wrong shape
    (tmp_path / "bad.cube").write_text("LUT_1D_SIZE 4\n" + "0 0 0\n" * 4)
    for kw in (dict(size=(32, 24)), dict(native_rgb=True), dict(deinterlace="frame"), dict(denoise=2), dict(devices=[0, 1]), dict(devices=[0, 1], row_split=True),
               dict(lut_bit_depth=12), dict(lut=str(tmp_path / "bad.cube")), dict(lut=str(tmp_path / "none.cube")), dict(lut=np.zeros((2, 2, 2))), dict(lut=7)):
        rc, enc = run("m.mp4", **{"lut": "hdr-to-sdr", **kw})
        assert rc == 1 and (enc is None or not enc.calls), kw
    # another layout than planar 4:2:0
    monkeypatch.setenv("FAKE_FB", str(w * h * 4))
    rc, enc = run("l.mp4", info=probe.VideoInfo(w, h, 30.0, "bt2020", "smpte2084", "bt2020nc", "yuv422p10le", "", "", 0, True, "eng", n, n / 30.0), lut="hdr-to-sdr")
    assert rc == 1 and (enc is None or not enc.calls)
