"""CPU: the downscaling source (mihevc_send_frame_scaled / mihevc_k_scale_source).  The numpy model of tests/scale_ref.py against hand-worked
cases; the table builder of hevc_amd/csrc/scale_taps.h against the model's Fraction tables, row for row; the kernel program of hevc_amd/csrc/kernels/scale.h
stepped on the CPU (tests/emu/scale.cpp) against the model, bit for bit, over random initial LDS in the three lane orders; the sanitizer program; the new entry
points without a device; the ABI struct; encode_file(size=) in front of a stand-in ffmpeg."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from hevc_amd import _lib
from tests import ingest_ref as IR
from tests import scale_ref as R
from tests import util
from tests.ingest_common import fake_ffmpeg, info, same_planes      # noqa: F401 (fake_ffmpeg: a fixture)
from tests.scale_common import CASES, DEPTHS, case_id, model, source

ROOT = Path(__file__).resolve().parents[1]


# ------------------------------------------------------------------------------------------------ 1. the model against hand-worked cases
def test_model_two_to_one_row():
    # centre aligned 2:1: pos = 2i + 1/2, taps k = 2i - 3 .. 2i + 4 at |t| = 1.75, 1.25, 0.75, 0.25: CR = -3/128, -9/128, 29/128, 111/128 (sum of the row 2):
    # c = CR * 2048
    first, coef, longest = R.table(32, 16, 2)
    assert longest == 8
    for i in range(16):
        assert first[i] == 2 * i - 3 and coef[i].tolist() == [-48, -144, 464, 1776, 1776, 464, -144, -48] + [0] * 8


def test_model_two_to_one_chroma_row():
    # co-sited 2:1 (p = 1): pos = ((4i + 1) 2Dn - Dn) / (4 Dn) = 2i + 1/4; taps k = 2i - 3 .. 2i + 4 at t = (pos - k) / 2 = 1.625, 1.125, 0.625, 0.125, -0.375,
    # -0.875, -1.375, -1.875.  In 1/2048 (the weights of a 2:1 row sum to 2): CR(0.125) = 1 - 2.5/64 + 1.5/512 = 1974/2048, CR(0.375) = 1490/2048,
    # CR(0.625) = 798/2048, CR(0.875) = 186/2048, CR(1.125) = -98/2048, CR(1.375) = -150/2048, CR(1.625) = -90/2048, CR(1.875) = -14/2048: nothing to round
    first, coef, longest = R.table(32, 16, 1)
    assert longest == 8
    for i in range(16):
        assert first[i] == 2 * i - 3 and coef[i].tolist() == [-90, -98, 798, 1974, 1490, 186, -150, -14] + [0] * 8
    assert sum([-90, -98, 798, 1974, 1490, 186, -150, -14]) == 4096


def test_model_one_to_one_is_a_single_tap():
    for p in (1, 2):
        first, coef, longest = R.table(40, 40, p)
        assert longest == 1 and first.tolist() == list(range(40)) and np.all(coef[:, 0] == 4096) and not coef[:, 1:].any()


@pytest.mark.parametrize("B,D", [(b, d) for b in (8, 10, 12, 16) for d in (8, 10)])
def test_model_one_to_one_is_the_source_conversion(B, D):
    f = IR.Format(420, 0, B, 0)
    for w, h in ((70, 38), (136, 72)):
        src = IR.random_source(f, w, h, w + B + D, full_word=True)
        assert not same_planes(R.scale(*src, B, w, h, D), IR.convert(f, *src, D))


def test_model_keeps_a_constant_plane_at_the_rails_too():
    for (sw, sh), (dw, dh) in CASES:
        for B, D in ((8, 8), (10, 8), (16, 10), (8, 10)):
            for val in (0, 1, (1 << B) - 1):
                y = np.full((sh, sw), val, R.src_dtype(B))
                c = np.full((sh // 2, sw // 2), val, R.src_dtype(B))
                want = (val << (D - B)) if D >= B else min((val + (1 << (B - D - 1))) >> (B - D), (1 << D) - 1)
                for p in R.scale(y, c, c, B, dw, dh, D):
                    assert np.all(p == want), ((sw, sh), (dw, dh), B, D, val)


def test_model_counts_the_clamped_taps_at_both_edges():
    # 2:1, 8 bit.  Output column 0 has taps k = -3 .. 4: four of them (-3, -2, -1, 0) read column 0: -48 - 144 + 464 + 1776 = 2048, half of the row.
    # Output column 1 (k = -1 .. 6) reads it twice: -48 - 144 = -192.  The right edge mirrors it.  Every row equal, so the vertical pass changes nothing
    S, Dn = 64, 32
    y = np.zeros((S, S), np.uint8)
    y[:, 0] = 200
    c = np.zeros((S // 2, S // 2), np.uint8)
    m = (R.filter_axis(y.astype(np.int64), S, Dn, 2, 1) + 128) >> 8
    assert m[0, :3].tolist() == [(2048 * 200 + 128) >> 8, -150, 0]          # (-192 * 200 + 128) / 256 = -149.5: rounds DOWN to -150
    out = R.scale(y, c, c, 8, Dn, Dn, 8)[0]
    assert out[5, :3].tolist() == [100, 0, 0] and not out[:, 2:].any()      # 1600 / 16 = 100; the negative T clamps to 0
    y = np.zeros((S, S), np.uint8)
    y[:, S - 1] = 200
    out = R.scale(y, c, c, 8, Dn, Dn, 8)[0]
    assert out[5, -3:].tolist() == [0, 0, 100] and not out[:, :-2].any()
    # vertically the same: row 0 counts four times at output row 0
    y = np.zeros((S, S), np.uint8)
    y[0, :] = 200
    assert R.scale(y, c, c, 8, Dn, Dn, 8)[0][:3, 7].tolist() == [100, 0, 0]
    # chroma, horizontally co-sited: column 0 of output 0 collects -90 - 98 + 798 + 1974 = 2584: (2584 * 200 + 128) >> 8 = 2019, (2019 * 4096 + 2^15) >> 16 = 126
    c = np.zeros((S // 2, S // 2), np.uint8)
    c[:, 0] = 200
    assert R.scale(np.zeros((S, S), np.uint8), c, c, 8, Dn, Dn, 8)[1][3, :2].tolist() == [126, 0]


def test_model_rounds_a_half_up_and_floors_a_negative_sum():
    # 1:1, 10 -> 8 bit: m = v << 4, T = 4096 m, n = 12 + 4 + 2: out = (v + 2) >> 2.  513 -> 128 (128.25), 514 -> 129 (128.5: up), 1023 -> 256 -> 255
    y = np.full((16, 16), 513, "<u2")
    y[0, 1], y[0, 2] = 514, 1023
    z = np.zeros((8, 8), "<u2")
    assert R.scale(y, z, z, 10, 16, 16, 8)[0][0, :3].tolist() == [128, 129, 255]
    # a negative sum: an 8-bit step edge at 2:1, columns 0 .. 15 are 0 and 16 .. 31 are 255; every row equal, so T = 4096 m.  Output i has taps k = 2i - 3 .. 2i + 4
    #   i = 6 (k = 9 .. 16): only k = 16 is lit: -48 * 255 = -12240; m = (-12240 + 128) / 256 = -47.3: rounds DOWN to -48; (-48 * 4096 + 2^15) / 2^16 = -2.5: down to
    #          -3, clamped to 0
    #   i = 7 (k = 11 .. 18): (464 - 144 - 48) * 255 = 69360; m = 271 (271.4); (271 * 4096 + 2^15) >> 16 = 17 (17.4)
    #   i = 8 (k = 13 .. 20): (1776 + 1776 + 464 - 144 - 48) * 255 = 975120; m = 3809 (3809.06 and the half); out = 238 (238.06 and the half)
    y = np.zeros((32, 32), np.uint8)
    y[:, 16:] = 255
    z = np.zeros((16, 16), np.uint8)
    m = (R.filter_axis(y.astype(np.int64), 32, 16, 2, 1) + 128) >> 8
    assert m[4, 5:9].tolist() == [0, -48, 271, 3809]
    assert R.scale(y, z, z, 8, 16, 16, 8)[0][4, 5:10].tolist() == [0, 0, 17, 238, 255]
    assert (-48 * 4096 + 32768) >> 16 == -3


# ------------------------------------------------------------------------------------------------ 2. scale_taps.h against the model's tables
@pytest.fixture(scope="module")
def emu():
    lib = util.stepped_library()
    lib.emu_scale.argtypes = [C.POINTER(_lib.ScaleSrc)] + [C.c_void_p] * 3 + [C.c_int] * 5 + [C.c_uint] + [C.c_void_p] * 3 + [C.POINTER(C.c_int)]
    lib.emu_scale_taps.argtypes = [C.c_int] * 3 + [C.c_void_p] * 2 + [C.POINTER(C.c_int)]
    lib.emu_scale_tile.argtypes = [C.POINTER(C.c_int)] * 3
    return lib


def axis_pairs():
    pairs = {(3840, 1920), (7680, 1920), (1920, 1280), (1000, 998), (16, 16), (64, 16)}
    for (sw, sh), (dw, dh) in CASES + [((3840, 2160), (1920, 1080)), ((200, 140), (100, 70)), ((150, 104), (100, 70)), ((400, 280), (100, 70))]:
        pairs |= {(sw, dw), (sh, dh), (sw // 2, dw // 2), (sh // 2, dh // 2)}
    return sorted(pairs)


@pytest.mark.parametrize("p", [1, 2])
def test_header_tables_equal_the_model(emu, p):
    for S, Dn in axis_pairs():
        first, coef, taps = np.zeros(Dn, np.int32), np.zeros((Dn, R.TAPS), np.int16), C.c_int()
        assert emu.emu_scale_taps(S, Dn, p, first.ctypes.data, coef.ctypes.data, C.byref(taps)) == 0, (S, Dn)
        want_first, want_coef, longest = R.table(S, Dn, p)
        assert np.array_equal(first, want_first) and np.array_equal(coef, want_coef) and taps.value == longest, (S, Dn)
        c = coef.astype(np.int64)
        assert np.all(c.sum(axis=1) == 4096) and np.abs(c).sum(axis=1).max() <= 6144 and longest <= 16, (S, Dn)
        assert np.all(np.diff(first) >= 0)
        assert S != Dn or longest == 1


def test_header_refuses_what_the_definition_excludes(emu):
    buf, taps = np.zeros(64 * 16, np.int32), C.c_int()
    for S, Dn, p in ((15, 16, 2), (65, 16, 2), (32, 16, 0), (32, 16, 3), (0, 0, 2)):
        assert emu.emu_scale_taps(S, Dn, p, buf.ctypes.data, buf.ctypes.data, C.byref(taps)) == -3, (S, Dn, p)


# ------------------------------------------------------------------------------------------------ 3. the kernel program stepped on the CPU
def emu_scale(emu, case, B, D, order=0, align=16, seed=1):
    (sw, sh), (dw, dh) = case
    want = model(case, B, D)
    out = [np.full(p.shape, 0x77, p.dtype) for p in want]
    stats = (C.c_int * 4)()
    rc = emu.emu_scale(C.byref(_lib.ScaleSrc(sw, sh, B)), *[p.ctypes.data for p in source(case, B)], dw, dh, D, order, align, seed, *[p.ctypes.data for p in out], stats)
    assert rc == 0, rc
    assert stats[0] == 0, f"{stats[0]} misaligned accesses"
    assert stats[1] == 0, f"{stats[1]} samples written outside the coded width"
    assert (stats[2], stats[3]) == (align, align)
    return same_planes(out, want)


def test_sizes_meet_the_tile_edges(emu):
    tw, th, rows = C.c_int(), C.c_int(), C.c_int()
    emu.emu_scale_tile(C.byref(tw), C.byref(th), C.byref(rows))
    assert 136 > tw.value and 136 % tw.value and 72 > th.value and 72 % th.value          # 136x72: more than one tile each way, partial tiles
    assert R.coded(70) == 72 and R.coded(38) == 40 and (R.coded(70) // 2) % 8 == 4         # 70x38: margin on both sides, a chroma row that ends with half a run
    assert rows.value >= 4 * th.value + 16


@pytest.mark.parametrize("B,D", DEPTHS)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_stepped_kernel_equals_model(emu, case, B, D):
    for order in (0, 1, 2):
        diff = emu_scale(emu, case, B, D, order, 16, seed=17 * order + B)
        assert not diff, (order, diff)


@pytest.mark.parametrize("align", [1, 4, 8])
@pytest.mark.parametrize("B,D", DEPTHS)
def test_stepped_kernel_with_misaligned_planes(emu, B, D, align):
    """the same grid on planes of the narrower alignment classes: every case and depth pair in the three lane orders"""
    for case in CASES:
        for order in (0, 1, 2):
            diff = emu_scale(emu, case, B, D, order, align, seed=align + 5 * order)
            assert not diff, (case, order, diff)


def test_stepped_kernel_clamps_values_above_the_declared_depth():
    assert max(int(p.max()) for p in source(CASES[2], 10)) > 60000          # what every 10-bit case above was fed


def test_stepped_kernel_under_address_sanitizer(tmp_path):
    """a stand-alone program (its own main, no python in the process): the table builder and the stepped kernel over source planes allocated to end with their last
    sample, every ratio, element type and alignment class.  A read past a plane ends it with the sanitizer's report"""
    exe = tmp_path / "scale_asan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-w", "-o", str(exe),
                    str(ROOT / "tests" / "emu" / "scale.cpp"), str(ROOT / "tests" / "scale_asan_main.cc")], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert p.stdout.strip() == "288 runs"


# ------------------------------------------------------------------------------------------------ 4. the entry points without a device
def scale_call(sw=128, sh=96, dw=64, dh=48, B=8, D=8, **over):
    src = R.random_source(sw, sh, B, 1)
    pw, ph = R.coded(dw), R.coded(dh)
    out = [np.zeros(s, R.out_dtype(D)) for s in ((ph, pw), (ph // 2, pw // 2), (ph // 2, pw // 2))]
    a = dict(src=_lib.ScaleSrc(sw, sh, B), y=src[0].ctypes.data, u=src[1].ctypes.data, v=src[2].ctypes.data, pitch_y=sw, pitch_c=sw // 2, dw=dw, dh=dh, D=D,
             oy=out[0].ctypes.data, ou=out[1].ctypes.data, ov=out[2].ctypes.data)
    a.update(over)
    rc = _lib.load().mihevc_k_scale_source(0, None if a["src"] is None else C.byref(a["src"]), a["y"], a["u"], a["v"], a["pitch_y"], a["pitch_c"], a["dw"], a["dh"], a["D"],
                                           a["oy"], a["ou"], a["ov"])
    del src, out
    return rc


def test_scale_source_rejects_bad_arguments():
    assert scale_call(src=None) == _lib.EINVAL
    for sw, sh, dw, dh in ((127, 96, 64, 48), (128, 95, 64, 48), (128, 96, 63, 48), (128, 96, 64, 47), (14, 96, 14, 48), (128, 14, 64, 14),      # odd, too small
                           (62, 96, 64, 48), (128, 46, 64, 48), (258, 96, 64, 48), (128, 194, 64, 48)):                                          # upscaling, beyond 4:1
        assert scale_call(sw, sh, dw, dh) == _lib.EINVAL, (sw, sh, dw, dh)
    for B in (7, 17, 0):
        assert scale_call(src=_lib.ScaleSrc(128, 96, B)) == _lib.EINVAL
    for i in range(5):
        src = _lib.ScaleSrc(128, 96, 8)
        src.reserved[i] = 1
        assert scale_call(src=src) == _lib.EINVAL
    assert scale_call(pitch_y=127) == _lib.EINVAL and scale_call(pitch_c=63) == _lib.EINVAL
    assert scale_call(D=9) == _lib.EINVAL and scale_call(D=12) == _lib.EINVAL
    for k in ("y", "u", "v", "oy", "ou", "ov"):
        assert scale_call(**{k: None}) == _lib.EINVAL, k


def test_send_frame_scaled_rejects_a_null_session():
    y = np.zeros((96, 128), np.uint8)
    assert _lib.load().mihevc_send_frame_scaled(None, C.byref(_lib.ScaleSrc(128, 96, 8)), y.ctypes.data, y.ctypes.data, y.ctypes.data, 128, 64, 0, 0) == _lib.EINVAL


@pytest.mark.skipif(_lib.load().mihevc_device_count() > 0, reason="a GPU is present")
def test_no_gpu_means_loud_failure():
    assert scale_call() == _lib.ENODEV and scale_call(B=10, D=10) == _lib.ENODEV
    assert scale_call(src=None) == _lib.EINVAL          # the arguments are judged first


def test_scale_src_layout_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mihevc.h"\nint main(void){printf("%zu %zu %zu\\n",'
                   "sizeof(mihevc_scale_src),offsetof(mihevc_scale_src,bit_depth),offsetof(mihevc_scale_src,reserved));return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(_lib.ScaleSrc), _lib.ScaleSrc.bit_depth.offset, _lib.ScaleSrc.reserved.offset] and got[0] == 32
    assert _lib.load().mihevc_abi_version() == 6
    assert {"mihevc_send_frame_scaled", "mihevc_k_scale_source"} <= set(_lib.EXPORTS)


# ------------------------------------------------------------------------------------------------ 5. encode_file(size=)
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

    def send_scaled(self, width, height, y, u, v, bit_depth=None, pts=None, asynchronous=False):
        self.calls.append((width, height, y.shape, u.shape, v.shape, str(y.dtype), bit_depth, pts))

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


def test_encode_file_with_a_size_asks_the_pipe_for_the_source_as_it_is(fake_ffmpeg, tmp_path, monkeypatch):
    from hevc_amd import encoder, mp4
    sw, sh, n = 128, 96, 3
    monkeypatch.setenv("FAKE_FRAMES", str(n))
    monkeypatch.setenv("FAKE_FB", str(sw * sh * 3 // 2 * 2))
    monkeypatch.setattr(encoder, "Encoder", StubEncoder)
    StubEncoder.made.clear()
    out = tmp_path / "o.mp4"
    assert encoder.encode_file(tmp_path / "a.mov", out, info("yuv420p10le", sw, sh, n), total_frames=n, size=(64, 48)) == 0
    argv = fake_ffmpeg.read_text().split("\n")[-2].split()
    assert argv[argv.index("-pix_fmt") + 1] == "yuv420p10le" and not {"-s", "-vf", "-filter:v"} & set(argv) and not any("scale" in a for a in argv)
    (enc,) = StubEncoder.made
    assert (enc.cfg.width, enc.cfg.height, enc.cfg.bit_depth) == (64, 48, 10)
    assert enc.calls == [(sw, sh, (sh, sw), (sh // 2, sw // 2), (sh // 2, sw // 2), "uint16", 10, i) for i in range(n)]
    data = out.read_bytes()
    start, end = 0, len(data)
    for name in ("moov", "trak", "tkhd"):
        _, start, end = [b for b in mp4.parse_boxes(data, start, end) if b[0] == name][0]
    assert (int.from_bytes(data[end - 8:end - 4], "big") >> 16, int.from_bytes(data[end - 4:end], "big") >> 16) == (64, 48)      # the track has the target size
    # the level follows the target size too: 64x48 is level 1 territory for the reference's table, 128x96 is not asked
    from hevc_amd.transcoder import calculate_apple_hevc_level
    small = info("yuv420p10le", 64, 48, n)
    assert enc.cfg.level_idc == int(round(float(calculate_apple_hevc_level(small)[0]) * 30))
    # another layout with size=: an error, not a silent conversion
    StubEncoder.made.clear()
    monkeypatch.setenv("FAKE_FB", str(sw * sh * 2 * 2))
    assert encoder.encode_file(tmp_path / "a.mov", tmp_path / "p.mp4", info("yuv422p10le", sw, sh, n), total_frames=n, size=(64, 48)) == 1
    assert not StubEncoder.made or not StubEncoder.made[0].calls
