"""CPU: source conversion (mihevc_send_frame_fmt / mihevc_k_convert_source).  The numpy model of tests/ingest_ref.py against hand-worked cases; the kernel
program of hevc_amd/csrc/kernels/ingest.h stepped on the CPU (tests/emu) against that model, bit for bit, for every layout and depth; the new entry points
without a device; the ABI struct; the pixel format table; y4m / yuv clips in the new layouts; the ffmpeg pipe front end with a stand-in ffmpeg."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from hevc_amd import _lib, probe, yuvio
from tests import ingest_ref as R
from tests import util
from tests.ingest_common import fake_ffmpeg, info, pix_fmt_asked, same_planes      # noqa: F401 (fake_ffmpeg: a fixture)

ROOT = Path(__file__).resolve().parents[1]


def src_format(f):
    return _lib.SrcFormat(f.chroma, f.semi_planar, f.bit_depth, f.msb_aligned)


# every combination of chroma, planar / semi-planar, source depth (msb- and lsb-aligned above 8 bit) and output depth
COMBOS = [R.Format(c, s, b, m) for c in (420, 422, 444) for s in (0, 1) for b in (8, 10, 12, 16) for m in ((0, 1) if b > 8 else (0,))]
SIZES = [(16, 16), (72, 40), (70, 38)]


def combo_id(f):
    return f"{f.chroma}{'sp' if f.semi_planar else 'p'}-{f.bit_depth}{'msb' if f.msb_aligned else ''}"


# ------------------------------------------------------------------------------------------------ 1. the model against hand-worked cases
def one_chroma(f, c, depth=8):
    """Cb of a source whose Cb plane is `c` (luma and Cr zero)"""
    c = np.asarray(c, R.src_dtype(f))
    h = c.shape[0] * (2 if f.chroma == 420 else 1)
    w = c.shape[1] * (1 if f.chroma == 444 else 2)
    return R.convert(f, np.zeros((h, w), R.src_dtype(f)), c, np.zeros_like(c), depth)[1][:h // 2, :w // 2]


def test_model_444_ramp_and_left_edge_clamp():
    f = R.Format(444, 0, 8, 0)
    ramp = np.tile(np.arange(16) * 10, (16, 1))              # c[r][x] = 10 x: (10 (2i-1) + 20 (2i) + 10 (2i+1)) * 2 / 8 = 20 i for i > 0
    out = one_chroma(f, ramp)
    assert out.shape == (8, 8)
    assert out[0].tolist() == [3] + [20 * i for i in range(1, 8)]      # i = 0: the left tap is column 0: (0 + 0 + 10) * 2 = 20, (20 + 4) >> 3 = 3
    spike = np.zeros((16, 16), int)
    spike[:, 0] = 80                                          # column 0 counts three times at i = 0 (left tap clamped, centre), never at i = 1
    assert one_chroma(f, spike)[0, :2].tolist() == [(2 * 3 * 80 + 4) >> 3, 0]
    spike = np.zeros((16, 16), int)
    spike[:, 1] = 80                                          # column 1: the right tap of i = 0 and the left tap of i = 1
    assert one_chroma(f, spike)[0, :3].tolist() == [20, 20, 0]


def test_model_a_half_rounds_up():
    f = R.Format(422, 0, 8, 0)
    c = np.zeros((16, 8), int)
    c[0, 0], c[1, 0] = 1, 2                                   # S = 3, k = 1: 1.5 -> 2
    c[2, 0], c[3, 0] = 1, 1                                   # S = 2: 1
    c[4, 0], c[5, 0] = 0, 1                                   # S = 1: 0.5 -> 1
    assert one_chroma(f, c)[:3, 0].tolist() == [2, 1, 1]
    y = np.full((16, 16), 513, "<u2")                         # 10 -> 8 bit luma: (513 + 2) >> 2 = 128; 514: 128.5 -> 129
    y[0, 1] = 514
    z = np.zeros((8, 8), "<u2")
    assert R.convert(R.Format(420, 0, 10, 0), y, z, z, 8)[0][0, :2].tolist() == [128, 129]


def test_model_p010_shift_saturation_widening_and_clamp():
    y = np.full((16, 16), (700 << 6) | 63, "<u2")             # P010: the value sits in the top ten bits; the low six are dropped
    uv = np.full((8, 16), 512 << 6, "<u2")
    out = R.convert(R.Format(420, 1, 10, 1), y, uv, None, 10)
    assert out[0][0, 0] == 700 and out[1][0, 0] == 512 and out[2][0, 0] == 512
    assert out[0].dtype == np.uint16 and out[1].shape == (8, 8)
    z = np.zeros((8, 8), "<u2")
    y = np.full((16, 16), 4095, "<u2")                        # 12 -> 10: (4095 + 2) >> 2 = 1024 -> saturates at 1023
    y[0, 1] = 4093                                            # (4093 + 2) >> 2 = 1023
    y[0, 2] = 4089                                            # 1022.75 -> 1022
    assert R.convert(R.Format(420, 0, 12, 0), y, z, z, 10)[0][0, :3].tolist() == [1023, 1023, 1022]
    y = np.full((16, 16), 65535, "<u2")                       # 16 -> 10: (65535 + 32) >> 6 = 1024 -> 1023; 16 -> 8: (65535 + 128) >> 8 = 256 -> 255
    assert R.convert(R.Format(420, 0, 16, 0), y, z, z, 10)[0][0, 0] == 1023
    assert R.convert(R.Format(420, 0, 16, 0), y, z, z, 8)[0][0, 0] == 255
    y8, z8 = np.full((16, 16), 255, np.uint8), np.zeros((8, 8), np.uint8)
    y8[0, 1] = 16
    assert R.convert(R.Format(420, 0, 8, 0), y8, z8, z8, 10)[0][0, :2].tolist() == [1020, 64]      # 8 -> 10: << 2
    y = np.full((16, 16), 1023, "<u2")
    y[0, 0], y[0, 1] = 1024, 65535                            # above the declared depth of an lsb-aligned plane: clamped to 1023
    assert R.convert(R.Format(420, 0, 10, 0), y, z, z, 10)[0][0, :3].tolist() == [1023, 1023, 1023]
    assert R.convert(R.Format(420, 0, 10, 0), y, z, z, 8)[0][0, :3].tolist() == [255, 255, 255]


def test_model_margin_replicates_the_last_column_and_row():
    f = R.Format(444, 0, 8, 0)
    y, u, v = R.random_source(f, 70, 38, 1)
    out = R.convert(f, y, u, v, 8)
    assert [p.shape for p in out] == [(40, 72), (20, 36), (20, 36)]
    assert np.array_equal(out[0][:38, :70], y)
    for p, (sh, sw) in zip(out, [(38, 70), (19, 35), (19, 35)]):
        assert np.all(p[:, sw:] == p[:, sw - 1:sw]) and np.all(p[sh:, :] == p[sh - 1:sh, :])


# ------------------------------------------------------------------------------------------------ 2. the kernel program stepped on the CPU
@pytest.fixture(scope="module")
def emu():
    lib = util.stepped_library()
    lib.emu_ingest.argtypes = [C.POINTER(_lib.SrcFormat)] + [C.c_void_p] * 3 + [C.c_int] * 5 + [C.c_void_p] * 3 + [C.POINTER(C.c_int)]
    lib.emu_ingest_tile.argtypes = [C.POINTER(C.c_int)] * 2
    return lib


def emu_convert(emu, f, src, w, h, depth, order=0, align=16):
    pw, ph = R.coded(w), R.coded(h)
    out = [np.full(s, 0x77, R.out_dtype(depth)) for s in ((ph, pw), (ph // 2, pw // 2), (ph // 2, pw // 2))]
    stats = (C.c_int * 4)()
    rc = emu.emu_ingest(C.byref(src_format(f)), *[None if p is None else p.ctypes.data for p in src], w, h, depth, order, align, *[p.ctypes.data for p in out], stats)
    assert rc == 0, rc
    assert stats[0] == 0, f"{stats[0]} misaligned chunk accesses"
    assert stats[1] == 0, f"{stats[1]} samples written outside the coded width"
    return out, (stats[2], stats[3])


def test_sizes_meet_the_tile_edges(emu):
    tw, th = C.c_int(), C.c_int()
    emu.emu_ingest_tile(C.byref(tw), C.byref(th))
    assert 72 % tw.value and 40 % th.value and 40 > th.value          # 72x40: coded = display, partial tiles; more than one tile row
    assert R.coded(70) == 72 and R.coded(38) == 40                    # 70x38: margin on both sides
    assert (R.coded(70) // 2) % 8 == 4                                # and a chroma row that ends with half a run


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("f", COMBOS, ids=combo_id)
def test_stepped_kernel_equals_model(emu, f, depth):
    for w, h in SIZES:
        src = R.random_source(f, w, h, w * h + depth + f.bit_depth)
        want = R.convert(f, *src, depth)
        for order in (0, 1, 2):
            got, al = emu_convert(emu, f, src, w, h, depth, order)
            assert al == (16, 16)
            assert not same_planes(got, want), (w, h, order, same_planes(got, want))


@pytest.mark.parametrize("align", [1, 4, 8])
@pytest.mark.parametrize("f,depth", [(R.Format(444, 0, 8, 0), 8), (R.Format(444, 1, 8, 0), 10), (R.Format(422, 0, 10, 0), 10), (R.Format(444, 1, 16, 1), 8),
                                     (R.Format(420, 1, 10, 1), 10)], ids=lambda v: combo_id(v) if isinstance(v, tuple) else str(v))
def test_stepped_kernel_narrow_load_paths(emu, f, depth, align):
    """base pointers one element off a 16-byte boundary and an odd pitch (align 1: element loads), or 4- / 8-byte alignment and no more: one case per
    element type and more; the wide paths must not be taken (the harness counts every chunk access that is not aligned to its size)"""
    for w, h in SIZES[1:]:
        src = R.random_source(f, w, h, 5 * w + align)
        got, al = emu_convert(emu, f, src, w, h, depth, 2, align)
        assert al == (align, align)
        assert not same_planes(got, R.convert(f, *src, depth)), (w, h, same_planes(got, R.convert(f, *src, depth)))


def test_stepped_kernel_clamps_values_above_the_declared_depth(emu):
    f = R.Format(422, 0, 10, 0)
    src = R.random_source(f, 72, 40, 3, full_word=True)
    assert max(int(p.max()) for p in src) > 60000
    for depth in (8, 10):
        got, _ = emu_convert(emu, f, src, 72, 40, depth)
        assert not same_planes(got, R.convert(f, *src, depth))


def test_stepped_kernel_under_address_sanitizer(tmp_path):
    """a stand-alone program (its own main, no python in the process): the stepped kernel over source planes allocated to end with their last sample, every layout,
    element type and alignment class.  A read past a plane ends it with the sanitizer's report"""
    exe = tmp_path / "ingest_asan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-w", "-o", str(exe),
                    str(ROOT / "tests" / "emu" / "ingest.cpp"), str(ROOT / "tests" / "ingest_asan_main.cc")], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert p.stdout.strip() == "720 runs"


# ------------------------------------------------------------------------------------------------ 3. the entry points without a device
def convert_args(f, w=64, h=48, depth=8, pitch_y=None, pitch_c=None):
    src = R.random_source(f, w, h, 1)
    pw, ph = R.coded(w), R.coded(h)
    out = [np.zeros(s, R.out_dtype(depth)) for s in ((ph, pw), (ph // 2, pw // 2), (ph // 2, pw // 2))]
    keep = src + out
    args = [None if p is None else p.ctypes.data for p in src] + [w, h, pitch_y or src[0].shape[1], pitch_c or src[1].shape[1], depth] + [p.ctypes.data for p in out]
    return args, keep


def test_convert_source_rejects_bad_arguments():
    lib = _lib.load()
    good = R.Format(422, 0, 10, 0)
    args, keep = convert_args(good)
    assert lib.mihevc_k_convert_source(0, None, *args) == _lib.EINVAL
    for bad in (R.Format(411, 0, 8, 0), R.Format(0, 0, 8, 0), R.Format(422, 0, 7, 0), R.Format(422, 0, 17, 0), R.Format(420, 1, 8, 1), R.Format(422, 2, 8, 0),
                R.Format(422, 0, 10, 2)):
        a, k = convert_args(good)
        assert lib.mihevc_k_convert_source(0, C.byref(src_format(bad)), *a) == _lib.EINVAL, bad
    for i in range(4):
        fmt = src_format(good)
        fmt.reserved[i] = 1
        assert lib.mihevc_k_convert_source(0, C.byref(fmt), *args) == _lib.EINVAL
    fmt = src_format(good)
    for w, h in ((63, 48), (64, 47)):
        a = list(args)
        a[3], a[4] = w, h
        assert lib.mihevc_k_convert_source(0, C.byref(fmt), *a) == _lib.EINVAL
    for k, v in ((5, 63), (6, 31)):                           # a pitch smaller than the plane
        a = list(args)
        a[k] = v
        assert lib.mihevc_k_convert_source(0, C.byref(fmt), *a) == _lib.EINVAL
    a, keep2 = convert_args(R.Format(444, 1, 8, 0))
    a[6] = 2 * 64 - 1                                         # an interleaved 4:4:4 row is twice the width
    assert lib.mihevc_k_convert_source(0, C.byref(src_format(R.Format(444, 1, 8, 0))), *a) == _lib.EINVAL
    a = list(args)
    a[7] = 9                                                  # output depth
    assert lib.mihevc_k_convert_source(0, C.byref(fmt), *a) == _lib.EINVAL
    for k in (0, 1, 2, 8, 9, 10):                             # a NULL plane
        a = list(args)
        a[k] = None
        assert lib.mihevc_k_convert_source(0, C.byref(fmt), *a) == _lib.EINVAL


def test_send_frame_fmt_rejects_a_null_session():
    lib = _lib.load()
    y = np.zeros((48, 64), np.uint16)
    assert lib.mihevc_send_frame_fmt(None, C.byref(src_format(R.Format(422, 0, 10, 0))), y.ctypes.data, y.ctypes.data, y.ctypes.data, 64, 32, 0, 0) == _lib.EINVAL


@pytest.mark.skipif(_lib.load().mihevc_device_count() > 0, reason="a GPU is present")
def test_no_gpu_means_loud_failure():
    lib = _lib.load()
    for f in (R.Format(422, 0, 10, 0), R.Format(420, 1, 8, 0)):
        args, keep = convert_args(f)
        assert lib.mihevc_k_convert_source(0, C.byref(src_format(f)), *args) == _lib.ENODEV


# ------------------------------------------------------------------------------------------------ 4. ABI
def test_src_format_layout_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mihevc.h"\nint main(void){printf("%zu %zu %zu %d %d\\n",'
                   "sizeof(mihevc_src_format),offsetof(mihevc_src_format,msb_aligned),offsetof(mihevc_src_format,reserved),MIHEVC_SRC_DEVICE,MIHEVC_SRC_ASYNC);return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(_lib.SrcFormat), _lib.SrcFormat.msb_aligned.offset, _lib.SrcFormat.reserved.offset, _lib.SRC_DEVICE, _lib.SRC_ASYNC]
    assert C.sizeof(_lib.SrcFormat) == 32
    lib = _lib.load()
    assert lib.mihevc_abi_version() == 6
    assert {"mihevc_send_frame_fmt", "mihevc_k_convert_source"} <= set(_lib.EXPORTS)


# ------------------------------------------------------------------------------------------------ 5. the pixel format table
def test_src_format_for_covers_the_name_table():
    assert len(R.FORMATS) == 3 * 2 + 3 * 5 + 9
    for name, f in R.FORMATS.items():
        got = _lib.src_format_for(name)
        assert got is not None, name
        assert (got.chroma, got.semi_planar, got.bit_depth, got.msb_aligned, list(got.reserved)) == (f.chroma, f.semi_planar, f.bit_depth, f.msb_aligned, [0] * 4), name
    for name in R.UNSUPPORTED + ("", None, "yuv420p10", "yuvj420p10le", "yuva420p", "p010be", "yuv440p", "gray"):
        assert _lib.src_format_for(name) is None, name


# ------------------------------------------------------------------------------------------------ 6. clips on disk
@pytest.mark.parametrize("chroma,depth", [(422, 8), (444, 10), (420, 12)])
def test_y4m_round_trip_in_the_new_layouts(tmp_path, chroma, depth):
    f = R.Format(chroma, 0, depth, 0)
    w, h, n = 48, 32, 3
    frames = [R.random_source(f, w, h, i) for i in range(n)]
    path = tmp_path / "c.y4m"
    yuvio.write_y4m(path, frames, w, h, fps=25, bit_depth=10 if depth > 8 else 8, chroma=chroma, src_depth=depth if depth > 8 else None)
    assert path.read_bytes().split(b"\n")[0].split()[-1] == (f"C{chroma}p{depth}" if depth > 8 else f"C{chroma}").encode()
    clip = yuvio.open_clip(path)
    try:
        assert (clip.width, clip.height, clip.fps, clip.n_frames, clip.bit_depth) == (w, h, 25.0, n, 10 if depth > 8 else 8)
        assert clip.src_format == src_format(f)
        got = list(clip.frames())
        assert len(got) == n
        for g, want in zip(got, frames):
            assert [p.shape for p in g] == list(R.plane_shapes(f, w, h))
            assert all(np.array_equal(a, b) for a, b in zip(g, want))
    finally:
        clip.close()


def test_plain_clips_open_as_before(tmp_path):
    w, h = 64, 48
    rng = np.random.default_rng(0)
    frames = [tuple(rng.integers(0, 256, s).astype(np.uint8) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2))) for _ in range(2)]
    path = tmp_path / "a.y4m"
    yuvio.write_y4m(path, frames, w, h)
    assert path.read_bytes().startswith(b"YUV4MPEG2 W64 H48 F30:1 Ip A1:1 C420jpeg\n")
    clip = yuvio.open_clip(path)
    assert clip.src_format is None and clip.bit_depth == 8 and clip.n_frames == 2 and clip.frame_bytes == w * h * 3 // 2
    assert all(np.array_equal(a, b) for g, want in zip(clip.frames(), frames) for a, b in zip(g, want))
    clip.close()
    path10 = tmp_path / "b.y4m"
    yuvio.write_y4m(path10, [tuple(p.astype(np.uint16) * 4 for p in frames[0])], w, h, bit_depth=10)
    assert path10.read_bytes().split(b"\n")[0].endswith(b" C420p10")
    clip = yuvio.open_clip(path10)
    assert clip.src_format is None and clip.bit_depth == 10 and clip.n_frames == 1
    clip.close()
    # the raw .yuv names of the existing tests
    for name, depth, hdr in (("d_64x64_30.yuv", 8, False), ("clip_64x48_30_10bit_hdr.yuv", 10, True), ("x_64x48_29.97fps_8bit_sdr.yuv", 8, False)):
        hh = int(name.split("x")[1].split("_")[0]) if name[0] != "x" else 48
        p = tmp_path / name
        p.write_bytes(bytes(64 * hh * 3 // 2 * (2 if depth > 8 else 1) * 2))
        clip = yuvio.open_clip(p)
        assert (clip.width, clip.height, clip.bit_depth, clip.hdr, clip.n_frames, clip.src_format) == (64, hh, depth, hdr, 2, None), name
        assert [q.shape for q in next(clip.frames())] == [(hh, 64), (hh // 2, 32), (hh // 2, 32)]
        clip.close()
    with pytest.raises(ValueError):
        yuvio.open_clip(tmp_path / "noname.yuv")
    bad = tmp_path / "m.y4m"
    bad.write_bytes(b"YUV4MPEG2 W64 H48 F30:1 Cmono\n")
    with pytest.raises(ValueError, match="unsupported chroma format"):
        yuvio.open_clip(bad)


def test_raw_yuv_names_take_chroma_and_depth_tokens(tmp_path):
    for name, f in (("a_32x16_30_422.yuv", R.Format(422, 0, 8, 0)), ("a_32x16_30_444_12bit.yuv", R.Format(444, 0, 12, 0)), ("a_32x16_30_16bit_hdr.yuv", R.Format(420, 0, 16, 0))):
        src = R.random_source(f, 32, 16, 2)
        p = tmp_path / name
        yuvio.write_yuv(p, [src], bit_depth=f.bit_depth)
        clip = yuvio.open_clip(p)
        assert clip.src_format == src_format(f) and clip.n_frames == 1 and clip.bit_depth == (10 if f.bit_depth > 8 else 8)
        assert all(np.array_equal(a, b) for a, b in zip(next(clip.frames()), src))
        clip.close()


# ------------------------------------------------------------------------------------------------ 7. the ffmpeg pipe front end
def test_pipe_clip_asks_for_the_probed_format(fake_ffmpeg, tmp_path, monkeypatch):
    monkeypatch.setenv("FAKE_FRAMES", "3")
    monkeypatch.setenv("FAKE_FB", str((64 * 48 + 2 * 32 * 48) * 2))
    clip = yuvio.open_any(tmp_path / "a.mov", info("yuv422p10le"))
    assert clip.bit_depth == 10 and clip.src_format == _lib.SrcFormat(422, 0, 10, 0)
    got = list(clip.frames())
    clip.close()
    assert pix_fmt_asked(fake_ffmpeg) == "yuv422p10le"
    assert len(got) == 3 and [p.shape for p in got[0]] == [(48, 64), (48, 32), (48, 32)] and got[0][0].dtype == np.dtype("<u2")
    monkeypatch.setenv("FAKE_FB", str(64 * 48 * 3 // 2))
    clip = yuvio.open_any(tmp_path / "a.mov", info("nv12"))
    got = list(clip.frames())
    clip.close()
    assert pix_fmt_asked(fake_ffmpeg) == "nv12" and clip.src_format == _lib.SrcFormat(420, 1, 8, 0)
    assert len(got) == 3 and [None if p is None else p.shape for p in got[0]] == [(48, 64), (24, 64), None]
    for pix in ("yuv420p", "gbrp", "yuyv422", "yuvj444p"):      # the session's own layout, formats the conversion does not cover, full range: planar 4:2:0
        clip = yuvio.open_any(tmp_path / "a.mov", info(pix))
        got = list(clip.frames())
        clip.close()
        assert pix_fmt_asked(fake_ffmpeg) == "yuv420p" and clip.src_format is None, pix
        assert len(got) == 3 and [p.shape for p in got[0]] == [(48, 64), (24, 32), (24, 32)]
    monkeypatch.setenv("FAKE_FB", str(64 * 48 * 3))
    clip = yuvio.open_any(tmp_path / "a.mov", info("gbrp10le"))     # an unknown deep format: 4:2:0 at 10 bit, as before
    assert len(list(clip.frames())) == 3 and pix_fmt_asked(fake_ffmpeg) == "yuv420p10le" and clip.src_format is None
    clip.close()
    clip = yuvio.open_any(tmp_path / "a.mov", info("yuv422p10le"), native_formats=False)      # a consumer without send_fmt (row split)
    assert len(list(clip.frames())) == 3 and pix_fmt_asked(fake_ffmpeg) == "yuv420p10le" and clip.src_format is None
    clip.close()
