"""CPU: frame-rate multiplication (mihevc_send_frame_interpolate / mihevc_k_mcfi_vectors / mihevc_k_mcfi_render).  The numpy model of
tests/mcfi_ref.py against a sample-by-sample restatement in Python ints and hand-worked cases; what the model does to pans; the programs of
hevc_amd/csrc/kernels/mcfi.h stepped on the CPU (tests/emu/mcfi.cpp) against the model, bit for bit, over random initial LDS in the three lane orders; their
divisions over the whole range; the sanitizer program; the new entry points without a device; the ABI struct; encode_file(interpolate=) in front of a stand-in
ffmpeg."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from hevc_amd import _lib
from tests import mcfi_ref as R
from tests import util
from tests.ingest_common import fake_ffmpeg, info, same_planes      # noqa: F401 (fake_ffmpeg: a fixture)
from tests.mcfi_common import FACTORS, KINDS, SIZES, extreme_fields, frames, model_picture, model_vectors, planes_of, plane_pointers, texture, wavy
from tests.test_deint_cpu import StubEncoder

ROOT = Path(__file__).resolve().parents[1]


# ------------------------------------------------------------------------------------------------ 1. the model against a restatement in Python ints
def clampi(v, lo, hi):
    return lo if v < lo else hi if v > hi else v


def scalar_vectors(cur, nxt, depth):
    """§6j for one frame pair, nothing vectorised, every index written out: -> v0, v, D as nested lists"""
    H, W = len(cur), len(cur[0])
    peak, sh = (1 << depth) - 1, depth - 8
    s8 = [[[min(int(f[y][x]), peak) >> sh for x in range(W)] for y in range(H)] for f in (cur, nxt)]
    hh = [[[(s[2 * y][2 * x] + s[2 * y][2 * x + 1] + s[2 * y + 1][2 * x] + s[2 * y + 1][2 * x + 1] + 2) >> 2 for x in range(W // 2)] for y in range(H // 2)] for s in s8]
    nbx, nby = (W + 7) // 8, (H + 7) // 8

    def sad(img, x0, y0, n, vx, vy):
        a, b = img
        hy, hx = len(a), len(a[0])
        return sum(abs(a[clampi(y0 + r - vy, 0, hy - 1)][clampi(x0 + c - vx, 0, hx - 1)] - b[clampi(y0 + r + vy, 0, hy - 1)][clampi(x0 + c + vx, 0, hx - 1)])
                   for r in range(n) for c in range(n))
    v0 = [[None] * nbx for _ in range(nby)]
    for by in range(nby):
        for bx in range(nbx):
            best = None
            for vy in range(-8, 9):
                for vx in range(-8, 9):
                    l1 = abs(vx) + abs(vy)
                    k = (sad(hh, 4 * bx - 2, 4 * by - 2, 8, vx, vy) + 2 * l1) * 2 ** 15 + l1 * 2 ** 9 + (vy + 8) * 17 + vx + 8
                    if best is None or k < best[0]:
                        best = (k, vx, vy)
            v1, best = best[1:], None
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    vx, vy = 2 * v1[0] + dx, 2 * v1[1] + dy
                    l1 = abs(vx) + abs(vy)
                    k = (sad(s8, 8 * bx - 4, 8 * by - 4, 16, vx, vy) + 4 * l1) * 2 ** 15 + l1 * 2 ** 9 + (dy + 2) * 5 + dx + 2
                    if best is None or k < best[0]:
                        best = (k, vx, vy)
            v0[by][bx] = best[1:]
    v = [[None] * nbx for _ in range(nby)]
    for by in range(nby):
        for bx in range(nbx):
            nine = [v0[clampi(by + j, 0, nby - 1)][clampi(bx + i, 0, nbx - 1)] for j in (-1, 0, 1) for i in (-1, 0, 1)]
            vm = tuple(sorted(n[k] for n in nine)[4] for k in (0, 1))
            zero = sad(s8, 8 * bx - 4, 8 * by - 4, 16, *vm) + 4 * (abs(vm[0]) + abs(vm[1])) > sad(s8, 8 * bx - 4, 8 * by - 4, 16, 0, 0)
            v[by][bx] = (0, 0) if zero else vm
    D = sum(abs(s8[0][y][x] - s8[1][y][x]) for y in range(H) for x in range(W))
    return v0, v, D


def scalar_sample(Cp, Np, v, f, j, x, y, chroma, peak):
    """one output sample of one plane of picture j of f (no cut), every index written out"""
    H, W = len(Cp), len(Cp[0])
    nby, nbx = len(v), len(v[0])
    bs, ps = (4, 8) if chroma else (8, 4)

    def at(F, r, c):
        return min(int(F[clampi(r, 0, H - 1)][clampi(c, 0, W - 1)]), peak)

    def fetch(F, px, py):
        xi, yi, fx, fy = px // ps, py // ps, px % ps, py % ps          # (floor division and a non-negative remainder)
        return (ps - fx) * (ps - fy) * at(F, yi, xi) + fx * (ps - fy) * at(F, yi, xi + 1) + (ps - fx) * fy * at(F, yi + 1, xi) + fx * fy * at(F, yi + 1, xi + 1)
    X, Y = x - bs // 2, y - bs // 2
    i0, j0 = X // bs, Y // bs
    ax, ay = X - bs * i0, Y - bs * j0
    num = 0
    for bj, wy in ((j0, bs - ay), (j0 + 1, ay)):
        for bi, wx in ((i0, bs - ax), (i0 + 1, ax)):
            vx, vy = v[clampi(bj, 0, nby - 1)][clampi(bi, 0, nbx - 1)]
            dx, dy = 2 * int(vx), 2 * int(vy)
            qx, qy = (8 * dx * j + f) // (2 * f), (8 * dy * j + f) // (2 * f)
            A = fetch(Cp, ps * x - qx, ps * y - qy)
            B = fetch(Np, ps * x + 4 * dx - qx, ps * y + 4 * dy - qy)
            num += wx * wy * ((f - j) * A + j * B)
    assert 0 <= num < 2 ** 23
    return (num + 512 * f) // (1024 * f)


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("kind", ["noise", "pan8", "pan36", "flat"])
def test_model_vectors_equal_the_restatement(depth, kind):
    c, n = frames((16, 16), depth, kind)
    v0, v, D = model_vectors((16, 16), depth, kind)
    s0, s, sD = scalar_vectors(c[0].tolist(), n[0].tolist(), depth)
    assert v0.tolist() == [[list(t) for t in row] for row in s0] and v.tolist() == [[list(t) for t in row] for row in s] and D == sD
    if kind == "flat":
        assert not v0.any() and D == 0          # every cost ties: the key yields the zero vector


def test_model_vectors_equal_the_restatement_with_partial_blocks():
    c, n = frames((26, 18), 8, "pan8")
    v0, v, D = R.vectors(c[0], n[0], 8)
    s0, s, sD = scalar_vectors(c[0].tolist(), n[0].tolist(), 8)
    assert v0.shape == (3, 4, 2) and v0.tolist() == [[list(t) for t in row] for row in s0] and v.tolist() == [[list(t) for t in row] for row in s] and D == sD


@pytest.mark.parametrize("depth", [8, 10])
def test_model_render_equals_the_restatement(depth):
    size = (70, 36)
    w, h = size
    c, n = frames(size, depth, "noise")
    rng = np.random.default_rng(depth)
    fields = extreme_fields(size) + [rng.integers(-R.VMAX, R.VMAX + 1, (R.blocks(h), R.blocks(w), 2)).astype(np.int16)]
    peak = (1 << depth) - 1
    for k, v in enumerate(fields):
        for f in FACTORS:
            for j in range(f):
                got = R.render(c, n, depth, f, j, v, 0, 0, 0)
                for plane in range(3):
                    ww, hh = (w, h) if plane == 0 else (w // 2, h // 2)
                    spots = [(0, 0), (ww - 1, 0), (0, hh - 1), (ww - 1, hh - 1), (ww // 2, hh // 2), (3, 4), (4, 3), (ww - 5, hh - 4), (int(rng.integers(ww)), int(rng.integers(hh)))]
                    for x, y in spots:
                        want = scalar_sample(c[plane].tolist(), n[plane].tolist(), v.tolist(), f, j, x, y, plane > 0, peak)
                        assert int(got[plane][y, x]) == want, (k, f, j, plane, x, y)


# ------------------------------------------------------------------------------------------------ 2. hand-worked cases
def display(planes, size):
    w, h = size
    return [p[:h, :w] if c == 0 else p[:h // 2, :w // 2] for c, p in enumerate(planes)]


@pytest.mark.parametrize("depth", [8, 10])
def test_picture_0_is_the_frame(depth):
    size = (70, 36)
    for kind in ("noise", "pan8", "object"):
        c, n = frames(size, depth, kind)
        want = [R.sample(p, depth) for p in c]
        for f in FACTORS:
            for thr in (0, 10):
                assert not same_planes(display(model_picture(size, depth, kind, f, 0, 0, thr), size), want)
            assert not same_planes(display(model_picture(size, depth, kind, f, 0, 1), size), want)
    for v in extreme_fields(size):          # whatever the field
        assert not same_planes(display(R.render(c, n, depth, 3, 0, v, 0, 0, 0), size), want)


def test_static_pictures_stay_as_they_are():
    size = (72, 72)
    f0 = planes_of(texture(72, 72, 8), 8, 0)
    v0, v, D = R.vectors(f0[0], f0[0], 8)
    assert not v0.any() and not v.any() and D == 0
    for f in FACTORS:
        for j in range(f):
            assert not same_planes(display(R.render(f0, f0, 8, f, j, v, D), size), list(f0))


@pytest.mark.parametrize("depth", [8, 10])
def test_a_cut_repeats_the_nearer_frame(depth):
    size = (70, 36)
    c, n = frames(size, depth, "cut")
    _, v, D = model_vectors(size, depth, "cut")
    assert R.is_cut(D, 10, *size) and not R.is_cut(D, 0, *size) and v.any()
    for f in FACTORS:
        for j in range(f):
            want = [R.sample(p, depth) for p in (c if 2 * j <= f else n)]
            assert not same_planes(display(model_picture(size, depth, "cut", f, j), size), want), (f, j)
    assert same_planes(display(model_picture(size, depth, "cut", 2, 1, 0, 0), size), [R.sample(p, depth) for p in c])          # threshold 0: no cut, a real picture


@pytest.mark.parametrize("depth", [8, 10])
def test_blend_at_factor_2_is_the_rounded_mean(depth):
    size = (70, 36)
    c, n = frames(size, depth, "noise")
    want = [(R.sample(a, depth) + R.sample(b, depth) + 1) >> 1 for a, b in zip(c, n)]
    assert not same_planes(display(model_picture(size, depth, "noise", 2, 1, 1), size), want)


def test_the_division_by_3072_floors():
    for num in (0, 1535, 1536, 3071 + 1536, 3072 + 1536 - 1, 2 ** 23 - 1):
        assert (num + 512 * 3) // (1024 * 3) == int((num + 1536) / 3072)


# ------------------------------------------------------------------------------------------------ 3. what the model does to pans
PAN_SIZE = (160, 128)
EXACT_PANS = [(8, -4), (-16, -28), (32, -32), (4, 0), (0, -20), (-32, 12)]
OTHER_PANS = [(36, 36), (-36, 12), (0, 36), (6, 2), (10, -6), (2, 2), (30, 14), (34, -22)]


def pan_case(d):
    """C, N and the true picture halfway of a wavy texture that moves by d"""
    (w, h), (dx, dy) = PAN_SIZE, d
    m = max(abs(dx), abs(dy))
    T = wavy(h + 2 * m, w + 2 * m, 9)
    c, n = (planes_of(T[m - k * dy:m - k * dy + h, m - k * dx:m - k * dx + w], 8, 0) for k in (0, 1))
    return c, n, T[m - dy // 2:m - dy // 2 + h, m - dx // 2:m - dx // 2 + w]


@pytest.mark.parametrize("d", EXACT_PANS, ids=str)
def test_pans_by_multiples_of_4_are_reproduced_exactly(d):
    """d = 4 v1 with v1 inside the level-1 range of +-8: the half-size images of C and N are shifts of each other by whole samples, level 1 finds v1 with SAD 0,
    level 0 keeps 2 v1, and 48 samples from every edge (the reach of the windows, the median and the overlap) picture 1 of 2 is the texture moved by d / 2.  A
    component of +-36 needs v1 = 9: level 1 has to end at +-8 off by one half-size sample and level 0 has to add 2; on no texture tried (box-filtered noise of
    5 .. 17 samples, waves of 25 .. 160 samples with and without detail) did every interior block do that: 36 is in OTHER_PANS below"""
    (w, h), (dx, dy) = PAN_SIZE, d
    c, n, mid = pan_case(d)
    _, v, D = R.vectors(c[0], n[0], 8)
    assert (v[5:-5, 5:-5] == np.array([dx // 2, dy // 2])).all()
    pic = R.render(c, n, 8, 2, 1, v, D, 0, 0)[0][:h, :w]
    assert np.array_equal(pic[48:-48, 48:-48], mid[48:-48, 48:-48])


def test_other_even_pans_beat_the_blend(capsys):
    """luma PSNR of picture 1 of 2 against the true picture halfway, 48 samples from every edge, mc and blend (99: equal).  The figures of DESIGN.md §6j, mc / blend
    in dB: (36, 36) 35.43 / 29.11; (-36, 12) 38.49 / 25.91; (0, 36) 48.18 / 27.71; (6, 2) 99 / 37.68; (10, -6) 99 / 34.00; (2, 2) 99 / 46.68; (30, 14) 99 / 31.80;
    (34, -22) 99 / 24.99"""
    (w, h), lines = PAN_SIZE, []
    for d in OTHER_PANS:
        c, n, mid = pan_case(d)
        _, v, D = R.vectors(c[0], n[0], 8)
        mc, bl = (util.psnr(R.render(c, n, 8, 2, 1, v, D, mode, 0)[0][48:h - 48, 48:w - 48], mid[48:-48, 48:-48]) for mode in (0, 1))
        lines.append(f"d = {d}: mc {mc:.2f} dB, blend {bl:.2f} dB")
        assert mc >= bl, lines[-1]
    with capsys.disabled():
        print("\n" + "\n".join(lines))


# ------------------------------------------------------------------------------------------------ 4. the programs stepped on the CPU
@pytest.fixture(scope="module")
def emu():
    lib = util.stepped_library()
    vp = C.c_void_p
    lib.emu_mcfi_vectors.argtypes = [vp, vp] + [C.c_int] * 5 + [C.c_uint, vp, vp, vp, C.POINTER(C.c_int)]
    lib.emu_mcfi_render.argtypes = [C.POINTER(_lib.Interpolate), C.c_int, C.POINTER(vp), C.POINTER(vp), vp, C.c_uint64] + [C.c_int] * 5 + [C.c_uint, vp, vp, vp, C.POINTER(C.c_int)]
    lib.emu_mcfi_tiles.argtypes = [C.POINTER(C.c_int)] * 4
    return lib


def emu_vectors(emu, c, n, size, depth, order=0, align=16, seed=1):
    nby, nbx = R.blocks(size[1]), R.blocks(size[0])
    v0, v, D, stats = np.full((nby, nbx, 2), 99, np.int16), np.full((nby, nbx, 2), 99, np.int16), C.c_uint64(1), (C.c_int * 4)()
    rc = emu.emu_mcfi_vectors(c[0].ctypes.data, n[0].ctypes.data, size[0], size[1], depth, order, align, seed, v0.ctypes.data, v.ctypes.data, C.addressof(D), stats)
    assert rc == 0, rc
    assert stats[0] == 0, f"{stats[0]} misaligned accesses"
    assert stats[2] == align
    return v0, v, D.value


def emu_render(emu, c, n, size, depth, f, j, v, D, mode=0, thr=10, order=0, align=16, seed=1):
    pw, ph = (size[0] + 7) & ~7, (size[1] + 7) & ~7
    out = [np.full(s, 0x77, R.dtype(depth)) for s in ((ph, pw), (ph // 2, pw // 2), (ph // 2, pw // 2))]
    stats = (C.c_int * 4)()
    rc = emu.emu_mcfi_render(C.byref(_lib.Interpolate(f, mode, thr)), j, plane_pointers(c), plane_pointers(n), None if v is None else v.ctypes.data, D, size[0], size[1],
                             depth, order, align, seed, *[p.ctypes.data for p in out], stats)
    assert rc == 0, rc
    assert stats[0] == 0, f"{stats[0]} misaligned accesses"
    assert stats[1] == 0, f"{stats[1]} samples written outside the coded width"
    assert (stats[2], stats[3]) == (align, align)
    return out


def test_sizes_meet_the_tile_edges(emu):
    sb, tw, th, lds = C.c_int(), C.c_int(), C.c_int(), (C.c_int * 3)()
    emu.emu_mcfi_tiles(C.byref(sb), C.byref(tw), C.byref(th), lds)
    assert R.blocks(72) == sb.value + 1 and tw.value < 72 < 2 * tw.value and 2 * th.value < 72 < 3 * th.value          # 72x72: one block more than a search tile
    assert tw.value < 138 // 2 < 2 * tw.value and th.value < 74 // 2 < 2 * th.value and (138 // 2) % 4 and (74 // 2) % 4  # 138x74: its chroma tiles, mid-block ends
    assert 70 % 8 and 36 % 8 and (70 // 2) % 4                                                                          # 70x36: partial blocks
    assert 4 * lds[0] <= 160 * 1024 and 4 * lds[1] <= 160 * 1024 and 2 * lds[2] <= 160 * 1024                           # workgroups that share a CU's 160 KB of LDS


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_stepped_search_and_field_equal_model(emu, size, depth):
    for kind in KINDS:
        c, n = frames(size, depth, kind)
        want = model_vectors(size, depth, kind)
        for order in (0, 1, 2):
            v0, v, D = emu_vectors(emu, c, n, size, depth, order, 16, seed=17 * order + depth)
            assert np.array_equal(v0, want[0]) and np.array_equal(v, want[1]) and D == want[2], (kind, order)


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_stepped_render_equals_model(emu, size, depth):
    i = 0
    for kind in KINDS:
        c, n = frames(size, depth, kind)
        _, v, D = model_vectors(size, depth, kind)
        for f in FACTORS:
            for j in range(f):
                for thr in (0, 10):
                    i += 1
                    diff = same_planes(emu_render(emu, c, n, size, depth, f, j, v, D, 0, thr, i % 3, 16, seed=i), model_picture(size, depth, kind, f, j, 0, thr))
                    assert not diff, (kind, f, j, thr, diff)
        diff = same_planes(emu_render(emu, c, n, size, depth, 3, 2, None, 0, 1, 10, i % 3, 16, seed=i), model_picture(size, depth, kind, 3, 2, 1))
        assert not diff, (kind, "blend", diff)


@pytest.mark.parametrize("align", [1, 4, 8, 16])
@pytest.mark.parametrize("depth", [8, 10])
def test_stepped_render_with_extreme_fields_and_misaligned_planes(emu, depth, align):
    """+-18 in every block and alternating signs: the windows' halo at the picture's corners and at every tile edge"""
    for size in SIZES:
        c, n = frames(size, depth, "noise")
        for k, v in enumerate(extreme_fields(size)):
            f = FACTORS[k % 3]
            j = 1 + k % (f - 1)
            diff = same_planes(emu_render(emu, c, n, size, depth, f, j, v, 0, 0, 0, k % 3, align, seed=align + k), R.render(c, n, depth, f, j, v, 0, 0, 0))
            assert not diff, (size, k, diff)


@pytest.mark.parametrize("align", [1, 4, 8])
@pytest.mark.parametrize("depth", [8, 10])
def test_stepped_search_with_misaligned_planes(emu, depth, align):
    for i, size in enumerate(SIZES):
        c, n = frames(size, depth, "noise")
        want = model_vectors(size, depth, "noise")
        v0, v, D = emu_vectors(emu, c, n, size, depth, i % 3, align, seed=align + i)
        assert np.array_equal(v0, want[0]) and np.array_equal(v, want[1]) and D == want[2], size


def test_stepped_kernels_clamp_values_above_the_declared_depth():
    assert max(int(p.max()) for f in frames(SIZES[1], 10, "noise") for p in f) > 60000          # what every 10-bit noise case above was fed


def test_stepped_divisions_are_exact_over_the_whole_range(emu):
    """(num + 512 f) / (1024 f) for every num below 2^23 and f = 2, 3, 4 (f = 3: a multiplication and a shift), and the floor division of the offsets for every
    d = 2v, |v| <= 18, and every j"""
    assert emu.emu_mcfi_div_check() == 0


def test_stepped_render_refuses_a_field_out_of_range(emu):
    size = (70, 36)
    c, n = frames(size, 8, "noise")
    for bad in (19, -19, 200):
        v = extreme_fields(size)[0]
        v[2, 3, 1] = bad
        out = [np.zeros((40, 72), np.uint8), np.zeros((20, 36), np.uint8), np.zeros((20, 36), np.uint8)]
        assert emu.emu_mcfi_render(C.byref(_lib.Interpolate(2, 0, 0)), 1, plane_pointers(c), plane_pointers(n), v.ctypes.data, 0, 70, 36, 8, 0, 16, 1,
                                   *[p.ctypes.data for p in out], (C.c_int * 4)()) == -3


def test_stepped_kernels_under_address_sanitizer(tmp_path):
    """a stand-alone program (its own main, no python in the process): the stepped programs over source planes allocated to end with their last sample, every
    size, element type and alignment class, searched fields and the extreme ones.  A read past a plane ends it with the sanitizer's report"""
    exe = tmp_path / "mcfi_asan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-w", "-o", str(exe),
                    str(ROOT / "tests" / "emu" / "mcfi.cpp"), str(ROOT / "tests" / "mcfi_asan_main.cc")], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert p.stdout.strip() == "160 runs"


# ------------------------------------------------------------------------------------------------ 5. the entry points without a device
def vectors_call(w=64, h=48, depth=8, **over):
    y = np.zeros((h, w), R.dtype(depth))
    nb = R.blocks(w) * R.blocks(h)
    v0, v, D = np.zeros(2 * nb, np.int16), np.zeros(2 * nb, np.int16), C.c_uint64()
    a = dict(cur=y.ctypes.data, next=y.ctypes.data, w=w, h=h, pitch=w, depth=depth, v0=v0.ctypes.data, v=v.ctypes.data, D=C.addressof(D))
    a.update(over)
    return _lib.load().mihevc_k_mcfi_vectors(0, a["cur"], a["next"], a["w"], a["h"], a["pitch"], a["depth"], a["v0"], a["v"], a["D"])


def render_call(w=64, h=48, depth=8, j=1, **over):
    fr = frames((w, h), depth, "flat") if (w, h) in SIZES else [[np.zeros(s, R.dtype(depth)) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2))]] * 2
    pw, ph = (w + 7) & ~7, (h + 7) & ~7
    out = [np.zeros(s, R.dtype(depth)) for s in ((ph, pw), (ph // 2, pw // 2), (ph // 2, pw // 2))]
    v = np.zeros((R.blocks(h), R.blocks(w), 2), np.int16)
    a = dict(m=_lib.Interpolate(2, 0, 10), j=j, cur=plane_pointers(fr[0]), next=plane_pointers(fr[1]), v=v.ctypes.data, D=0, w=w, h=h, pitch_y=w, pitch_c=w // 2, depth=depth,
             oy=out[0].ctypes.data, ou=out[1].ctypes.data, ov=out[2].ctypes.data)
    a.update(over)
    if isinstance(a["v"], np.ndarray):
        a["v"] = a["v"].ctypes.data
    return _lib.load().mihevc_k_mcfi_render(0, None if a["m"] is None else C.byref(a["m"]), a["j"], a["cur"], a["next"], a["v"], a["D"], a["w"], a["h"], a["pitch_y"],
                                            a["pitch_c"], a["depth"], a["oy"], a["ou"], a["ov"])


def test_vectors_rejects_bad_arguments():
    for w, h in ((63, 48), (64, 47), (14, 48), (64, 14)):      # odd, too small
        assert vectors_call(w=w, h=h, pitch=64) == _lib.EINVAL, (w, h)
    assert vectors_call(pitch=63) == _lib.EINVAL
    for depth in (9, 12, 16, 0):
        assert vectors_call(depth=depth) == _lib.EINVAL
    for k in ("cur", "next", "v0", "v", "D"):
        assert vectors_call(**{k: None}) == _lib.EINVAL, k


def test_render_rejects_bad_arguments():
    for w, h in ((63, 48), (64, 47), (14, 48), (64, 14)):
        assert render_call(w=w, h=h, pitch_y=64, pitch_c=32) == _lib.EINVAL, (w, h)
    assert render_call(pitch_y=63) == _lib.EINVAL and render_call(pitch_c=31) == _lib.EINVAL
    for depth in (9, 12, 16, 0):
        assert render_call(depth=depth) == _lib.EINVAL
    assert render_call(m=None) == _lib.EINVAL
    for t in ((1, 0, 10), (5, 0, 10), (0, 0, 10), (2, 2, 10), (2, -1, 10), (2, 0, -1), (2, 0, 256)):
        assert render_call(m=_lib.Interpolate(*t)) == _lib.EINVAL, t
    for k in range(5):
        m = _lib.Interpolate(2, 0, 10)
        m.reserved[k] = 1
        assert render_call(m=m) == _lib.EINVAL
    assert render_call(j=-1) == _lib.EINVAL and render_call(j=2) == _lib.EINVAL and render_call(m=_lib.Interpolate(4, 0, 10), j=4) == _lib.EINVAL
    for k in ("cur", "next", "oy", "ou", "ov", "v"):
        assert render_call(**{k: None}) == _lib.EINVAL, k
    y = np.zeros((48, 64), np.uint8)
    for k in ("cur", "next"):
        assert render_call(**{k: (C.c_void_p * 3)(y.ctypes.data, None, y.ctypes.data)}) == _lib.EINVAL, k
    for bad in (19, -19, 32767, -32768):          # a component outside [-18, 18], in any block
        for where in ((0, 0, 0), (5, 7, 1), (2, 3, 0)):
            v = np.zeros((6, 8, 2), np.int16)
            v[where] = bad
            assert render_call(v=v) == _lib.EINVAL, (bad, where)


def test_send_frame_interpolate_rejects_a_null_session():
    y = np.zeros((48, 64), np.uint8)
    assert _lib.load().mihevc_send_frame_interpolate(None, C.byref(_lib.Interpolate(2, 0, 10)), y.ctypes.data, y.ctypes.data, y.ctypes.data, 64, 32, 0, 0) == _lib.EINVAL


@pytest.mark.skipif(_lib.load().mihevc_device_count() > 0, reason="a GPU is present")
def test_no_gpu_means_loud_failure():
    assert vectors_call() == _lib.ENODEV and vectors_call(depth=10, h=50) == _lib.ENODEV
    assert render_call() == _lib.ENODEV and render_call(m=_lib.Interpolate(3, 1, 0), j=2, v=None) == _lib.ENODEV          # (blend takes no field)
    v = np.full((6, 8, 2), 18, np.int16)
    assert render_call(v=v) == _lib.ENODEV
    assert vectors_call(pitch=63) == _lib.EINVAL and render_call(j=2) == _lib.EINVAL          # the arguments are judged first


def test_interpolate_layout_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mihevc.h"\nint main(void){printf("%zu %zu %zu %zu %zu\\n",'
                   "sizeof(mihevc_interpolate),offsetof(mihevc_interpolate,factor),offsetof(mihevc_interpolate,mode),"
                   "offsetof(mihevc_interpolate,scene_threshold),offsetof(mihevc_interpolate,reserved));return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    M = _lib.Interpolate
    assert got == [C.sizeof(M), M.factor.offset, M.mode.offset, M.scene_threshold.offset, M.reserved.offset] and got == [32, 0, 4, 8, 12]
    assert _lib.load().mihevc_abi_version() == 6
    assert {"mihevc_send_frame_interpolate", "mihevc_k_mcfi_vectors", "mihevc_k_mcfi_render"} <= set(_lib.EXPORTS)


def test_interpolate_mode():
    m = _lib.interpolate_mode(3, "blend", 0)
    assert (m.factor, m.mode, m.scene_threshold) == (3, 1, 0) and tuple(m.reserved) == (0,) * 5
    assert (_lib.interpolate_mode(2).mode, _lib.interpolate_mode(2).scene_threshold) == (0, 10)
    for bad in ((1,), (5,), (2.0,), (True,), ("2",), (2, "mci"), (2, "mc", -1), (2, "mc", 256), (2, "mc", 1.5)):
        with pytest.raises(ValueError):
            _lib.interpolate_mode(*bad)


# ------------------------------------------------------------------------------------------------ 6. encode_file(interpolate=)
class InterpolateStub(StubEncoder):
    """gives the pictures a session would: `factor` for the frame before at every call but the first, one at flush"""

    def send_interpolate(self, y, u, v, factor=2, mode='mc', scene_threshold=10, asynchronous=False, pts=None):
        self.sent += factor if any(c[0] == "interpolate" for c in self.calls) else 0
        self.calls.append(("interpolate", y.shape, u.shape, str(y.dtype), factor, mode, scene_threshold, pts))

    def flush(self):
        self.sent += 1 if self.calls and self.calls[0][0] == "interpolate" else 0


def test_encode_file_interpolate_in_front_of_the_pipe(fake_ffmpeg, tmp_path, monkeypatch):
    from hevc_amd import encoder
    from hevc_amd.transcoder import calculate_apple_hevc_level
    import copy
    w, h, n = 64, 48, 4
    monkeypatch.setenv("FAKE_FRAMES", str(n))
    monkeypatch.setenv("FAKE_FB", str(w * h * 3 // 2))
    monkeypatch.setattr(encoder, "Encoder", InterpolateStub)
    seen = []

    def run(out, pix="yuv420p", **kw):
        StubEncoder.made.clear()
        seen.clear()
        rc = encoder.encode_file(tmp_path / "a.mov", tmp_path / out, info(pix, w, h, n), total_frames=n, progress_callback=lambda name, done, total: seen.append((done, total)), **kw)
        return rc, (StubEncoder.made[0] if StubEncoder.made else None)

    for f in FACTORS:
        for mode in ("mc", "blend"):
            rc, enc = run("f.mp4", interpolate=f, interp_mode=mode)
            argv = fake_ffmpeg.read_text().split("\n")[-2].split()
            assert rc == 0 and not any("minterpolate" in a or "fps=" in a for a in argv)          # the pipe is asked for the frames as they are
            assert enc.calls == [("interpolate", (h, w), (h // 2, w // 2), "uint8", f, mode, 10, f * i) for i in range(n)]
            assert enc.out == f * (n - 1) + 1 and seen[-1] == (f * (n - 1) + 1, f * (n - 1) + 1)   # pictures, and the progress total counts them
            fast = copy.copy(info("yuv420p", w, h, n))
            fast.fps = 30.0 * f
            assert enc.cfg.fps_num / enc.cfg.fps_den == 30.0 * f and enc.cfg.level_idc == int(round(float(calculate_apple_hevc_level(fast)[0]) * 30))
    for kw in ({}, dict(interpolate=None)):
        rc, enc = run("h.mp4", **kw)
        assert rc == 0 and enc.calls == [("plain", (h, w), i) for i in range(n)] and enc.cfg.fps_num / enc.cfg.fps_den == 30.0, kw
    for kw in (dict(deinterlace="frame"), dict(size=(32, 24)), dict(native_rgb=True), dict(devices=[0, 1]), dict(devices=[0, 1], row_split=True), dict(denoise=2),
               dict(lut="hdr-to-sdr"), dict(interpolate=1), dict(interpolate=5), dict(interpolate=2.0), dict(interpolate=True), dict(interp_mode="mci")):
        rc, enc = run("m.mp4", **{"interpolate": 2, **kw})
        assert rc == 1 and (enc is None or not enc.calls), kw
    monkeypatch.setenv("FAKE_FB", str(w * h * 2))
    rc, enc = run("l.mp4", pix="yuv422p", interpolate=2)
    assert rc == 1 and (enc is None or not enc.calls)
