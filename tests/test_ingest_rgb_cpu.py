"""CPU: RGB source conversion (mihevc_send_frame_rgb / mihevc_k_convert_rgb).  The numpy model of tests/ingest_rgb_ref.py against hand-worked cases and against
the definition evaluated in exact rationals; the kernel program of hevc_amd/csrc/kernels/ingest_rgb.h stepped on the CPU (tests/emu) against that model, bit for
bit, for every layout, component order, sample type and depth; the host's integer coefficients; the new entry points without a device; the ABI struct; the
pixel format table; the ffmpeg pipe front end with a stand-in ffmpeg."""
import ctypes as C
import functools
import itertools
import math
import subprocess
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

from hevc_amd import _lib, probe, yuvio
from tests import ingest_rgb_ref as R
from tests import util
from tests.ingest_common import fake_ffmpeg, pix_fmt_asked, same_planes      # noqa: F401 (fake_ffmpeg: a fixture)
from tests.ingest_common import info as common_info

ROOT = Path(__file__).resolve().parents[1]
MATRICES, DEPTHS, OUT_DEPTHS = (1, 5, 6, 9), (8, 10, 12, 16), (8, 10)
SIZES = [(16, 16), (72, 40), (70, 38)]


def rgb_format(f, matrix=0, full=None):
    return _lib.RgbFormat(f.layout, f.r, f.g, f.b, f.sample, f.bit_depth, matrix, 0 if full is None else 2 if full else 1)


def planar(depth, sample=0):
    return R.Format(0, 0, 1, 2, sample, depth)


def flat(f, rgb, w=16, h=16):
    """a picture of one colour (sample values, or floats) in the layout of f"""
    dt = R.src_dtype(f)
    if f.layout == 0:
        planes = [None] * 3
        for i, v in zip((f.r, f.g, f.b), rgb):
            planes[i] = np.full((h, w), v, dt)
        return planes
    p = np.zeros((h, w, f.layout), dt)
    for i, v in zip((f.r, f.g, f.b), rgb):
        p[:, :, i] = v
    return [p.reshape(h, w * f.layout)]


# ------------------------------------------------------------------------------------------------ 1. the model against hand-worked cases
@pytest.mark.parametrize("full", [False, True], ids=["limited", "full"])
@pytest.mark.parametrize("matrix", MATRICES)
def test_model_white_black_and_grey(matrix, full):
    for B, D in itertools.product(DEPTHS, OUT_DEPTHS):
        f, top, unit = planar(B), (1 << B) - 1, 1 << (D - 8)
        for v, want_y in ((top, (1 << D) - 1 if full else 235 * unit), (0, 0 if full else 16 * unit), (1 << (B - 1), None)):
            y, cb, cr = R.convert(f, flat(f, (v, v, v)), matrix, full, D)
            if want_y is None:      # mid-grey: the scale alone, rounded half up
                sy = Fraction((1 << D) - 1, top) if full else Fraction(219 * unit, top)
                want_y = int(sy * v + Fraction(1, 2)) + (0 if full else 16 * unit)
            assert np.all(y == want_y), (B, D, v, int(y[0, 0]), want_y)
            assert np.all(cb == 1 << (D - 1)) and np.all(cr == 1 << (D - 1)), (B, D, v, int(cb[0, 0]), int(cr[0, 0]))


@pytest.mark.parametrize("matrix", MATRICES)
def test_model_pure_blue_and_red_reach_the_chroma_peak(matrix):
    for B, D in itertools.product(DEPTHS, OUT_DEPTHS):
        f, top = planar(B), (1 << B) - 1
        assert np.all(R.convert(f, flat(f, (0, 0, top)), matrix, False, D)[1] == 240 << (D - 8)), (B, D)
        assert np.all(R.convert(f, flat(f, (top, 0, 0)), matrix, False, D)[2] == 240 << (D - 8)), (B, D)
        assert np.all(R.convert(f, flat(f, (top, top, 0)), matrix, False, D)[1] == 16 << (D - 8)), (B, D)       # yellow: the other end of Cb


def test_model_a_half_rounds_up_in_luma():
    # BT.709, full range, B = D = 8: s = 1, S = 16, m[0] = (13933, 46871, 4732) (0.2126, 0.7152, 0.0722 times 65536, rounded; they sum to 65536)
    assert R.coefficients(1, True, 8, 8) == ([[13933, 46871, 4732], [-7509, -25259, 32768], [32768, -29763, -3005]], 16)
    f = planar(8)
    # 13933 * 86 + 46871 * 238 = 1198238 + 11155298 = 12353536 = 188.5 * 65536: the half goes up
    assert 13933 * 86 + 46871 * 238 == 188 * 65536 + 32768
    assert R.convert(f, flat(f, (86, 238, 0)), 1, True, 8)[0][0, 0] == 189
    assert R.convert(f, flat(f, (86, 237, 0)), 1, True, 8)[0][0, 0] == 188          # 187.78
    assert R.convert(f, flat(f, (86, 238, 1)), 1, True, 8)[0][0, 0] == 189          # 188.57


def test_model_left_tap_clamp_and_taps():
    # BT.709, full range, B = D = 8: the Cb coefficient of blue is 32768 = 2^15, S + 3 = 19
    f = planar(8)
    z = np.zeros((16, 16), np.uint8)
    b = z.copy()
    b[:, 0] = 80        # column 0 counts three times at i = 0 (left tap clamped, centre twice), never at i = 1: T = 2 rows * 3 * 80 * 2^15 = 30 * 2^19
    assert R.convert(f, [z, z, b], 1, True, 8)[1][0, :3].tolist() == [128 + 30, 128, 128]
    b = z.copy()
    b[:, 1] = 80        # column 1: the right tap of i = 0 and the left tap of i = 1: 2 rows * 80 * 2^15 = 10 * 2^19 each
    assert R.convert(f, [z, z, b], 1, True, 8)[1][0, :3].tolist() == [138, 138, 128]
    b = z.copy()
    b[0, 2] = 80        # one row only, centre tap of i = 1: 2 * 80 * 2^15 = 10 * 2^19
    assert R.convert(f, [z, z, b], 1, True, 8)[1][:2, :3].tolist() == [[128, 138, 128], [128, 128, 128]]
    r = z.copy()
    r[:, 1] = 80        # red lowers Cb: T = 2 * 80 * -7509 = -1201440, (T + 2^18) >> 19 = floor(-1.79) = -2 at i = 0 and i = 1: the shift floors
    assert R.convert(f, [r, z, z], 1, True, 8)[1][0, :3].tolist() == [126, 126, 128]


def test_model_margin_replicates_the_last_column_and_row():
    f = R.FORMATS["rgb24"]
    out = R.convert(f, R.random_source(f, 70, 38, 1), 6, False, 10)
    assert [p.shape for p in out] == [(40, 72), (20, 36), (20, 36)] and out[0].dtype == np.uint16
    for p, (sh, sw) in zip(out, [(38, 70), (19, 35), (19, 35)]):
        assert np.all(p[:, sw:] == p[:, sw - 1:sw]) and np.all(p[sh:, :] == p[sh - 1:sh, :])


def test_model_float_rule():
    f32, f16 = planar(0, 2), planar(0, 1)
    bits = lambda *b: np.array(b, np.uint32).view(np.float32)
    x = np.array([np.nan, -np.nan, -1.0, -0.0, 0.0, 1.0, 1.5, np.inf, -np.inf, 0.5, 1e-30], np.float32)
    assert R.sample(x, f32).tolist() == [0, 0, 0, 0, 0, 65535, 65535, 65535, 0, 32768, 0]       # 0.5 * 65535 = 32767.5: the tie goes to the even 32768
    # float32 products that land on a tie: 0x3ec001c0 * 65535 rounds to 24576.5 and 0x3f00e901 * 65535 to 33000.5; both go DOWN to the even integer
    ties = bits(0x3EC001C0, 0x3F00E901)
    assert (ties * np.float32(65535)).tolist() == [24576.5, 33000.5]
    assert R.sample(ties, f32).tolist() == [24576, 33000]
    # the product is rounded to float32 before rint: 0.1f = 0x3dcccccd times 65535 is 6553.50009... exactly but 6553.5 as a float32, a tie, and goes to the
    # even 6554; 0x3dccccc0 * 65535 = 6553.4937 as a float32: 6553
    assert (bits(0x3DCCCCCD, 0x3DCCCCC0) * np.float32(65535)).tolist() == [6553.5, 6553.49365234375]
    assert R.sample(bits(0x3DCCCCCD, 0x3DCCCCC0), f32).tolist() == [6554, 6553]
    # halves are widened exactly, subnormals included: 0x0400 = 2^-14 (the smallest normal) * 65535 = 3.99994 -> 4; subnormals 0x0200 = 2^-15 -> 2.0,
    # 0x0100 = 2^-16 -> 0.99998 -> 1, 0x03ff = 1023 * 2^-24 -> 3.996 -> 4, 0x0001 = 2^-24 -> 0.0039 -> 0
    h = np.array([0x0400, 0x0200, 0x0100, 0x03FF, 0x0001, 0x3800, 0x3C00, 0x7C00, 0xFC00, 0x7E00, 0xFE00, 0x8200, 0x3C01], np.uint16).view(np.float16)
    assert R.sample(h, f16).tolist() == [4, 2, 1, 4, 0, 32768, 65535, 65535, 0, 0, 0, 0, 65535]
    # through the whole conversion: a float picture equals the 16-bit picture of its sample values
    src = R.random_source(f32, 32, 16, 5)
    as16 = [R.sample(p, f32).astype("<u2") for p in src]
    for a, b in zip(R.convert(f32, src, 9, False, 10), R.convert(planar(16), as16, 9, False, 10)):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------ 2. the model against the definition in exact rationals
def exact_check(matrix, full, B, D):
    """|model - exact| <= 0.5 + 1.5 * 2^(min(B, D) - 16) output steps, everywhere: half a step for the one rounding, and three coefficient roundings of at
    most half a unit each, times v <= 2^B, over 2^S = 2^(16 + max(0, B - D)).  A bound derived from the definition, not tuned"""
    rng = np.random.default_rng(B * 100 + D * 10 + matrix)
    top = (1 << B) - 1
    w, h = 64, 66
    planes = [rng.integers(0, top + 1, (h, w)).astype(np.int64) for _ in range(3)]        # 64 x 64 random pixels = 4096 ...
    for i, corner in enumerate(itertools.product((0, top), repeat=3)):                    # ... and the eight cube corners, 8 x 2 pixels each, below them
        for p, v in zip(planes, corner):
            p[64:, 8 * i:8 * i + 8] = v
    f = planar(B)
    model = [p[:h, :w].astype(np.int64) for p in R.convert(f, [p.astype(R.src_dtype(f)) for p in planes], matrix, full, D)]
    rows, (sy, sc, oy, oc) = R.rows(matrix), R.scales(full, B, D)
    bound, peak = Fraction(1, 2) + Fraction(3, 2) * Fraction(1 << min(B, D), 1 << 16), (1 << D) - 1
    worst = Fraction(0)

    def compare(got, coeffs, taps, offset):
        """got: the model's plane; exact value = sum of coeffs[c] * taps[c] + offset, clipped to 0 .. peak; with one common denominator in integers"""
        nonlocal worst
        den = 1
        for c in coeffs:
            den = den * c.denominator // math.gcd(den, c.denominator)
        num = sum(int(c * den) * t for c, t in zip(coeffs, taps)) + int(offset * den)          # int64: |num| < 2^50
        num = np.clip(num, 0, peak * den)
        err = np.abs(got * den - num)                                                           # in 1 / den output steps
        assert err.max() * bound.denominator <= bound.numerator * den, (matrix, full, B, D, float(Fraction(int(err.max()), int(den))), float(bound))
        worst = max(worst, Fraction(int(err.max()), int(den)))

    compare(model[0], [x * sy for x in rows[0]], planes, oy)
    for c in (1, 2):
        taps = []
        for p in planes:
            left = np.concatenate([p[:, :1], p[:, 1:-1:2]], axis=1)
            hs = left + 2 * p[:, 0::2] + p[:, 1::2]
            taps.append(hs[0::2] + hs[1::2])
        compare(model[c][:h // 2, :w // 2], [x * sc / 8 for x in rows[c]], taps, oc)
    return worst, bound


@pytest.mark.parametrize("full", [False, True], ids=["limited", "full"])
@pytest.mark.parametrize("matrix", MATRICES)
def test_model_against_exact_rationals(matrix, full):
    for B, D in itertools.product(DEPTHS, OUT_DEPTHS):
        worst, bound = exact_check(matrix, full, B, D)
        assert Fraction(1, 4) < worst <= bound          # and the check is alive: a rounding error of some size is there


# ------------------------------------------------------------------------------------------------ 3. the kernel program stepped on the CPU
@pytest.fixture(scope="module")
def emu():
    lib = util.stepped_library()
    lib.emu_ingest_rgb.argtypes = [C.POINTER(_lib.RgbFormat)] + [C.c_void_p] * 3 + [C.c_int] * 5 + [C.c_void_p] * 3 + [C.POINTER(C.c_int)]
    lib.emu_ingest_rgb_tile.argtypes = [C.POINTER(C.c_int)] * 2
    lib.emu_ingest_rgb_matrix.argtypes = [C.c_int] * 4 + [C.POINTER(C.c_int)] * 2
    return lib


def plane_ptrs(src):
    return [p.ctypes.data for p in src] + [None] * (3 - len(src))


def emu_convert(emu, f, src, w, h, matrix, full, depth, order=0, align=16):
    pw, ph = R.coded(w), R.coded(h)
    out = [np.full(s, 0x77, R.out_dtype(depth)) for s in ((ph, pw), (ph // 2, pw // 2), (ph // 2, pw // 2))]
    stats = (C.c_int * 4)()
    rc = emu.emu_ingest_rgb(C.byref(rgb_format(f, matrix, full)), *plane_ptrs(src), w, h, depth, order, align, *[p.ctypes.data for p in out], stats)
    assert rc == 0, rc
    assert stats[0] == 0, f"{stats[0]} misaligned accesses"
    assert stats[1] == 0, f"{stats[1]} samples written outside the coded width"
    return out, stats[2]


def test_host_coefficients_equal_the_rational_ones(emu):
    """the integer arithmetic of ingest_rgb_matrix against fractions.Fraction, every matrix, range and depth pair (B = 9 and 14 too)"""
    for matrix, full, B, D in itertools.product(MATRICES, (0, 1), range(8, 17), OUT_DEPTHS):
        m, S = (C.c_int * 9)(), C.c_int()
        assert emu.emu_ingest_rgb_matrix(matrix, full, B, D, m, C.byref(S)) == 0
        want, want_s = R.coefficients(matrix, bool(full), B, D)
        assert (list(m), S.value) == ([x for row in want for x in row], want_s), (matrix, full, B, D)
    assert emu.emu_ingest_rgb_matrix(2, 0, 8, 8, (C.c_int * 9)(), C.byref(C.c_int())) == -3


def test_sizes_meet_the_tile_edges(emu):
    tw, th = C.c_int(), C.c_int()
    emu.emu_ingest_rgb_tile(C.byref(tw), C.byref(th))
    assert (tw.value, th.value) == (256, 32)
    assert 40 > th.value and 40 % th.value                            # 72x40: coded = display; more than one tile row, the second partial
    assert 72 % 16 == 8                                               # a luma row that ends with half a block, and its chroma row with half a run
    assert R.coded(70) == 72 and R.coded(38) == 40                    # 70x38: margin on both sides


# every layout with every component order: the six orders of three planes and of three elements, and for four elements the four named ones plus two with
# the unused element inside the pixel
ORDERS = ([(0, p) for p in itertools.permutations(range(3))] + [(3, p) for p in itertools.permutations(range(3))] +
          [(4, p) for p in ((0, 1, 2), (2, 1, 0), (1, 2, 3), (3, 2, 1), (0, 2, 3), (3, 1, 0))])
KINDS = [(0, b) for b in DEPTHS] + [(1, 0), (2, 0)]                    # (sample, bit depth)
COMBOS = [R.Format(layout, *rgb, s, b) for layout, rgb in ORDERS for s, b in KINDS if not (s and layout)]


def combo_id(f):
    return f"{'planar' if not f.layout else 'packed%d' % f.layout}-{f.r}{f.g}{f.b}-{('u%d' % f.bit_depth, 'f16', 'f32')[f.sample]}"


@pytest.mark.parametrize("f", COMBOS, ids=combo_id)
def test_stepped_kernel_equals_model(emu, f):
    n = COMBOS.index(f)
    for k, (depth, (w, h)) in enumerate(itertools.product(OUT_DEPTHS, SIZES)):
        matrix, full = MATRICES[(n + k) % 4], bool((n + k) // 4 % 2)          # every matrix and both ranges, spread over the grid
        src = R.random_source(f, w, h, w * h + depth + n)
        want = R.convert(f, src, matrix, full, depth)
        for order in (0, 1, 2):
            got, al = emu_convert(emu, f, src, w, h, matrix, full, depth, order)
            assert al == 16
            assert not same_planes(got, want), (w, h, depth, matrix, full, order, same_planes(got, want))


@pytest.mark.parametrize("matrix", MATRICES)
def test_stepped_kernel_every_matrix_range_and_depth(emu, matrix):
    for full, B, D in itertools.product((False, True), DEPTHS, OUT_DEPTHS):
        f = R.Format(3, 2, 1, 0, 0, B) if B in (8, 16) else R.Format(0, 2, 0, 1, 0, B)
        src = R.random_source(f, 70, 38, B + D)
        got, _ = emu_convert(emu, f, src, 70, 38, matrix, full, D, 2)
        assert not same_planes(got, R.convert(f, src, matrix, full, D)), (full, B, D)


@pytest.mark.parametrize("align", [16, 8, 4, 1])
@pytest.mark.parametrize("name", ["gbrp", "gbrp10le", "rgb24", "bgra", "rgb48le", "rgba64le", "gbrpf32le", "f16"])
def test_stepped_kernel_alignment_classes(emu, name, align):
    """base pointers one element off a 16-byte boundary and an odd pitch (align 1: element loads), or 4- / 8-byte alignment and no more; the wide paths must
    not be taken there (the harness counts every access that is not aligned to its size)"""
    f = planar(0, 1) if name == "f16" else R.FORMATS[name]
    for w, h in SIZES[1:]:
        src = R.random_source(f, w, h, 5 * w + align)
        got, al = emu_convert(emu, f, src, w, h, 1, False, 10, 2, align)
        assert al == (4 if align == 1 and f.sample == 2 else align)      # a float32 plane one element off is still 4-byte aligned
        assert not same_planes(got, R.convert(f, src, 1, False, 10)), (w, h, same_planes(got, R.convert(f, src, 1, False, 10)))


def test_stepped_kernel_clamps_and_special_floats(emu):
    f = R.FORMATS["gbrp10le"]
    src = R.random_source(f, 72, 40, 3, full_word=True)                 # values above the declared depth
    assert max(int(p.max()) for p in src) > 60000
    for depth in OUT_DEPTHS:
        got, _ = emu_convert(emu, f, src, 72, 40, 5, True, depth)
        assert not same_planes(got, R.convert(f, src, 5, True, depth))
    # every half there is, as the three planes of one picture (65536 = 256 x 256 bit patterns, each plane a different order)
    f16 = planar(0, 1)
    every = np.arange(65536, dtype=np.uint16)
    src = [every.reshape(256, 256).view(np.float16), every[::-1].reshape(256, 256).view(np.float16), np.roll(every, 12345).reshape(256, 256).view(np.float16)]
    src = [np.ascontiguousarray(p) for p in src]
    got, _ = emu_convert(emu, f16, src, 256, 256, 1, True, 10)
    assert not same_planes(got, R.convert(f16, src, 1, True, 10))
    # float32: the ties, the edges of the clamp, subnormals, NaN and infinities of both signs in luma-visible places
    f32 = planar(0, 2)
    special = np.array([0x3EC001C0, 0x3F00E901, 0x3F000000, 0x3DCCCCC0, 0x7FC00000, 0xFFC00000, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x3F800001,
                        0x3F7FFFFF, 0x37800080, 0x38000040, 0xBF800000, 0x7F800001], np.uint32).view(np.float32)
    src = [np.ascontiguousarray(np.tile(np.roll(special, k), (16, 1))) for k in (0, 5, 11)]
    got, _ = emu_convert(emu, f32, src, 16, 16, 1, True, 10)
    assert not same_planes(got, R.convert(f32, src, 1, True, 10))


def test_stepped_kernel_under_address_sanitizer(tmp_path):
    """a stand-alone program (its own main, no python in the process): the stepped kernel over source planes allocated to end with their last sample, every
    layout, element type and alignment class.  A read past a plane ends it with the sanitizer's report"""
    exe = tmp_path / "ingest_rgb_asan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-w", "-o", str(exe),
                    str(ROOT / "tests" / "emu" / "ingest_rgb.cpp"), str(ROOT / "tests" / "ingest_rgb_asan_main.cc")], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert p.stdout.strip() == "192 runs"


# ------------------------------------------------------------------------------------------------ 4. the entry points without a device
def convert_args(f, w=64, h=48, depth=8, pitch=None):
    src = R.random_source(f, w, h, 1)
    pw, ph = R.coded(w), R.coded(h)
    out = [np.zeros(s, R.out_dtype(depth)) for s in ((ph, pw), (ph // 2, pw // 2), (ph // 2, pw // 2))]
    args = plane_ptrs(src) + [w, h, pitch or src[0].shape[1], depth] + [p.ctypes.data for p in out]
    return args, src + out


def test_convert_rgb_rejects_bad_arguments():
    lib = _lib.load()
    good = R.FORMATS["gbrp10le"]
    args, keep = convert_args(good)
    call = lambda fmt, a=args: lib.mihevc_k_convert_rgb(0, None if fmt is None else C.byref(fmt), *a)
    assert call(None) == _lib.EINVAL

    def bad(**fields):
        fmt = rgb_format(good, 1, False)
        for k, v in fields.items():
            setattr(fmt, k, v)
        return fmt
    for fields in (dict(layout=1), dict(layout=2), dict(layout=5), dict(layout=-1),                     # the layout
                   dict(r=3), dict(g=-1), dict(r=0), dict(b=0), dict(layout=3, r=3), dict(layout=4, b=4),  # indices out of range or used twice
                   dict(bit_depth=7), dict(bit_depth=17), dict(bit_depth=0),                             # integer depths
                   dict(sample=3), dict(sample=-1), dict(sample=1), dict(sample=2, bit_depth=16),       # floats carry depth 0
                   dict(sample=1, bit_depth=0, layout=3), dict(sample=2, bit_depth=0, layout=4, r=2, g=1, b=0),      # floats are planar only
                   dict(matrix=0), dict(matrix=2), dict(matrix=7), dict(matrix=-1),                     # no session to follow here
                   dict(range=0), dict(range=3), dict(range=-1)):
        assert call(bad(**fields)) == _lib.EINVAL, fields
    for i in range(4):
        fmt = bad()
        fmt.reserved[i] = 1
        assert call(fmt) == _lib.EINVAL
    fmt = bad()
    for w, h in ((63, 48), (64, 47), (14, 48)):
        a = list(args)
        a[3], a[4] = w, h
        assert call(fmt, a) == _lib.EINVAL
    a = list(args)
    a[5] = 63                                                 # a pitch smaller than the row
    assert call(fmt, a) == _lib.EINVAL
    a = list(args)
    a[6] = 9                                                  # output depth
    assert call(fmt, a) == _lib.EINVAL
    for k in (0, 1, 2, 7, 8, 9):                              # a NULL plane
        a = list(args)
        a[k] = None
        assert call(fmt, a) == _lib.EINVAL, k
    a = list(args)
    a[1] += 1                                                 # a 16-bit plane at an odd address
    assert call(fmt, a) == _lib.EINVAL
    packed = rgb_format(R.FORMATS["bgra"], 1, False)
    a, keep2 = convert_args(R.FORMATS["bgra"])
    b = list(a)
    b[5] = 4 * 64 - 1                                         # a packed row is layout * width elements
    assert call(packed, b) == _lib.EINVAL
    b = list(a)
    b[0] = None
    assert call(packed, b) == _lib.EINVAL


def test_send_frame_rgb_rejects_a_null_session():
    lib = _lib.load()
    y = np.zeros((48, 64), np.uint16)
    assert lib.mihevc_send_frame_rgb(None, C.byref(rgb_format(R.FORMATS["gbrp10le"], 1, False)), y.ctypes.data, y.ctypes.data, y.ctypes.data, 64, 0, 0) == _lib.EINVAL


@pytest.mark.skipif(_lib.load().mihevc_device_count() > 0, reason="a GPU is present")
def test_no_gpu_means_loud_failure():
    lib = _lib.load()
    for name in ("gbrp10le", "bgra", "gbrpf32le"):
        args, keep = convert_args(R.FORMATS[name])            # a packed source has no second and third plane: valid
        assert lib.mihevc_k_convert_rgb(0, C.byref(rgb_format(R.FORMATS[name], 9, True)), *args) == _lib.ENODEV


# ------------------------------------------------------------------------------------------------ 5. ABI
def test_rgb_format_layout_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    fields = ["layout", "r", "g", "b", "sample", "bit_depth", "matrix", "range", "reserved"]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mihevc.h"\nint main(void){printf("%zu' + " %zu" * len(fields) + '\\n",sizeof(mihevc_rgb_format),' +
                   ",".join(f"offsetof(mihevc_rgb_format,{n})" for n in fields) + ");return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(_lib.RgbFormat)] + [getattr(_lib.RgbFormat, n).offset for n in fields]
    assert C.sizeof(_lib.RgbFormat) == 48
    lib = _lib.load()
    assert lib.mihevc_abi_version() == 6
    assert {"mihevc_send_frame_rgb", "mihevc_k_convert_rgb"} <= set(_lib.EXPORTS)
    assert lib.mihevc_send_frame_rgb and lib.mihevc_k_convert_rgb


# ------------------------------------------------------------------------------------------------ 6. the pixel format table
def test_rgb_format_for_covers_the_name_table():
    assert len(R.FORMATS) == 7 + 2 + 8 + 4
    for name, f in R.FORMATS.items():
        got = _lib.rgb_format_for(name)
        assert got is not None, name
        assert got == rgb_format(f), (name, got)
        assert list(got.reserved) == [0] * 4 and got.matrix == 0 and got.range == 0
        assert _lib.src_format_for(name) is None, name
        back = [n for n in R.FORMATS if _lib.rgb_format_for(n) == got]          # and back: the names that share a layout, nothing else
        assert name in back and all(R.FORMATS[n] == f for n in back)
    assert _lib.rgb_format_for("GBRP10LE", matrix=9, range=2) == rgb_format(R.FORMATS["gbrp10le"], 9, True)
    for name in R.UNSUPPORTED + ("", None, "gbrp10", "gbrp11le", "rgb48", "rgba64be", "gbrpf16le", "rgb8", "bgr4", "xrgb", "rgbx"):
        assert _lib.rgb_format_for(name) is None, name
    assert _lib.rgb_format_for("gbrp").frame_bytes(64, 48) == 64 * 48 * 3 and _lib.rgb_format_for("bgra64le").frame_bytes(64, 48) == 64 * 48 * 8
    assert _lib.rgb_format_for("gbrpf32le").plane_shapes(64, 48) == [(48, 64)] * 3 and _lib.rgb_format_for("rgb24").plane_shapes(64, 48) == [(48, 192)]


# ------------------------------------------------------------------------------------------------ 7. the ffmpeg pipe front end
info = functools.partial(common_info, matrix="gbr")


def test_pipe_clip_asks_for_rgb_only_when_told_to(fake_ffmpeg, tmp_path, monkeypatch):
    monkeypatch.setenv("FAKE_FRAMES", "3")
    monkeypatch.setenv("FAKE_FB", str(64 * 48 * 3 * 2))
    clip = yuvio.open_any(tmp_path / "a.mov", info("gbrp10le"), rgb_formats=True)
    assert clip.bit_depth == 10 and clip.rgb_format == _lib.rgb_format_for("gbrp10le") and clip.src_format is None
    got = list(clip.frames())
    clip.close()
    assert pix_fmt_asked(fake_ffmpeg) == "gbrp10le"
    assert len(got) == 3 and [p.shape for p in got[0]] == [(48, 64)] * 3 and got[0][0].dtype == np.dtype("<u2")
    monkeypatch.setenv("FAKE_FB", str(64 * 48 * 4))
    clip = yuvio.open_any(tmp_path / "a.mov", info("bgr0"), rgb_formats=True)
    got = list(clip.frames())
    clip.close()
    assert pix_fmt_asked(fake_ffmpeg) == "bgr0" and clip.rgb_format == _lib.rgb_format_for("bgr0") and clip.bit_depth == 8
    assert len(got) == 3 and [p.shape for p in got[0]] == [(48, 256)] and got[0][0].dtype == np.uint8
    monkeypatch.setenv("FAKE_FB", str(64 * 48 * 3 * 4))
    clip = yuvio.open_any(tmp_path / "a.mov", info("gbrpf32le"), rgb_formats=True)      # floats: a 10-bit session
    got = list(clip.frames())
    clip.close()
    assert pix_fmt_asked(fake_ffmpeg) == "gbrpf32le" and clip.bit_depth == 10 and got[0][2].dtype == np.dtype("<f4") and got[0][2].shape == (48, 64)
    # without the option the request is what it was: planar 4:2:0 at the depth the name spells
    for pix, asked, fb in (("gbrp10le", "yuv420p10le", 64 * 48 * 3), ("bgr0", "yuv420p", 64 * 48 * 3 // 2), ("gbrp", "yuv420p", 64 * 48 * 3 // 2)):
        monkeypatch.setenv("FAKE_FB", str(fb))
        clip = yuvio.open_any(tmp_path / "a.mov", info(pix))
        got = list(clip.frames())
        clip.close()
        assert pix_fmt_asked(fake_ffmpeg) == asked and clip.rgb_format is None and clip.src_format is None, pix
        assert len(got) == 3 and [p.shape for p in got[0]] == [(48, 64), (24, 32), (24, 32)]
    # with it, formats outside the table and Y'CbCr sources are untouched
    monkeypatch.setenv("FAKE_FB", str(64 * 48 * 3 // 2))
    for pix in ("gbrap", "rgb565le", "pal8", "yuv420p"):
        clip = yuvio.open_any(tmp_path / "a.mov", info(pix), rgb_formats=True)
        assert len(list(clip.frames())) == 3 and pix_fmt_asked(fake_ffmpeg) == "yuv420p" and clip.rgb_format is None, pix
        clip.close()
    monkeypatch.setenv("FAKE_FB", str((64 * 48 + 2 * 32 * 48) * 2))
    clip = yuvio.open_any(tmp_path / "a.mov", info("yuv422p10le"), rgb_formats=True)
    assert len(list(clip.frames())) == 3 and pix_fmt_asked(fake_ffmpeg) == "yuv422p10le" and clip.rgb_format is None and clip.src_format is not None
    clip.close()
