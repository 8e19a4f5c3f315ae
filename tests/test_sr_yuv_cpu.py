"""CPU: the Y'CbCr input of the learned super-resolution without a device.  1. two facts of the numpy model tests/sr_yuv_ref.py and what its
edge cases are worth; 2. the stepped k_sr_from_yuv bit for bit against the model; 3. the stepped network over a Y'CbCr source against the stepped network fed the
model's 16-bit R'G'B'; 4. sr_target_size; 5. what encode_file refuses before a session is made, and what it no longer refuses; 6. the stand-alone
AddressSanitizer / UBSan program; 7. the stage entry without a device."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from hevc_amd import _lib
from tests import sr_common as S
from tests import sr_yuv_common as Q
from tests import sr_yuv_ref as Y
from tests import util

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def emu():
    return util.stepped_library()


# ------------------------------------------------------------------------------------------------ 1. the model itself
@pytest.mark.parametrize("B", [8, 10, 12])
def test_neutral_chroma_gives_grey_for_every_luma(B):
    """Cb = Cr = 2^(B-1): R = G = B for every Y, limited and full, every matrix"""
    h, w = 4, 1 << B
    y = np.tile(np.arange(w), (h, 1))
    c = np.full((h // 2, w // 2), 1 << (B - 1))
    for matrix in (1, 5, 6, 9):
        for full in (False, True):
            r, g, b = Y.rgb16((y, c, c), B, matrix, full)
            assert np.array_equal(r, g) and np.array_equal(g, b)
            assert r.min() == 0 and r.max() == 65535 and np.all(np.diff(r[0]) >= 0)


@pytest.mark.parametrize("scale", [4, 2])
def test_padding_channels_are_exactly_zero(scale):
    real = 12 if scale == 2 else 3
    for kind in Q.KINDS:
        t = Q.want(kind, 18, 14, 10, 6, False, scale)
        assert t.shape == ((7, 9, 32) if scale == 2 else (14, 18, 32))
        assert not t[:, :, real:].any() and t[:, :, :real].any()


def test_unshuffle_places_every_sample():
    """scale 2 holds exactly the halves of scale 4: channel c 4 + dy 2 + dx at (y, x) is component c at (2y + dy, 2x + dx)"""
    a, b = Q.want("random", 18, 14, 8, 1, True, 4), Q.want("random", 18, 14, 8, 1, True, 2)
    for c in range(3):
        for dy in range(2):
            for dx in range(2):
                assert np.array_equal(b[:, :, c * 4 + dy * 2 + dx], a[dy::2, dx::2, c])


@pytest.mark.parametrize("clamp", ["right", "top", "bottom"])
def test_edge_pictures_see_a_dropped_clamp(clamp):
    """the `edges` source exists for the clamps at column W/2 - 1, row H/2 - 1 and row 0.  With one of them dropped (the neighbour past the edge taken from
    the other side of the plane) the model's tensor moves in this many elements; every count must be above 0 for the edge pictures to be worth running.
    At 8 bit, matrix 6, limited range, scale 4 the counts at 4x4 / 18x14 / 34x16 / 66x34 are: right 8 / 37 / 43 / 91, top 5 / 40 / 79 / 155, bottom
    4 / 40 / 77 / 154 (the run prints them for every depth)."""
    for w, h in Q.SIZES:
        for B in (8, 10, 12):
            src = Q.source("edges", w, h, B)
            moved = int(np.count_nonzero(Y.input_tensor(src, B, 6, False, 4) != Y.input_tensor(src, B, 6, False, 4, grid=Y.grid_without(clamp))))
            print(f"{clamp} clamp dropped at {w}x{h}, {B} bit: {moved} elements move")
            assert moved > 0, (w, h, B)


def test_random_sources_reach_above_the_depth():
    for B in (10, 12):
        assert max(int(p.max()) for p in Q.source("random", 34, 16, B)) > (1 << B) - 1


# ------------------------------------------------------------------------------------------------ 2. the stepped kernel
@pytest.mark.parametrize("case", Q.CASES, ids=Q.case_id)
def test_stepped_kernel_is_the_model(emu, case):
    Q.check_case(emu, "emu_", case)


def test_stepped_kernel_in_every_thread_order(emu):
    src = Q.source("random", 66, 34, 10)
    for order in (0, 1, 2):
        for scale in (4, 2):
            got = Q.run_from_yuv(emu, "emu_", src, 10, 9, False, scale, pitch_extra=(3, 5), off_one=True, order=order)
            assert np.array_equal(got, Q.want("random", 66, 34, 10, 9, False, scale))


# ------------------------------------------------------------------------------------------------ 3. composition
@pytest.mark.parametrize("scale", [4, 2])
def test_stepped_network_over_yuv_equals_the_network_fed_the_models_rgb(emu, scale):
    """both sides run the same launches over the same input tensor, so the three half planes are equal bit for bit"""
    w, h, B, matrix = 12, 20, 8, 6
    src = Q.source("random", w, h, B)
    _, flat = S.net_weights(1, scale)
    model = _lib.SrModel(scale, 1)
    fmt, planes = Q.rgb16_planes(src, B, matrix, False)
    a = np.zeros((3, h * scale, w * scale), np.uint16)
    b = np.zeros_like(a)
    emu.emu_sr_network.argtypes = [C.POINTER(_lib.SrModel), C.c_void_p, C.c_size_t, C.POINTER(_lib.RgbFormat), C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_uint]
    assert emu.emu_sr_network(C.byref(model), util.ptr(flat), flat.size, C.byref(fmt), w, h, *map(util.ptr, planes), util.ptr(a), 0, 1) == 0
    emu.emu_sr_network_yuv.argtypes = [C.POINTER(_lib.SrModel), C.c_void_p, C.c_size_t, C.POINTER(_lib.SrYuv)] + [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_uint]
    yuv = _lib.SrYuv(w, h, B, matrix, 0)
    assert emu.emu_sr_network_yuv(C.byref(model), util.ptr(flat), flat.size, C.byref(yuv), *map(util.ptr, src), w, w // 2, util.ptr(b), 0, 1) == 0
    assert a.any() and np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------ 4. sr_target_size
def test_sr_target_size():
    from hevc_amd.encoder import sr_target_size
    assert sr_target_size(640, 480, 4, "auto") == (1440, 1080)
    assert sr_target_size(854, 480, 4, "auto") == (1920, 1080)
    assert sr_target_size(1280, 720, 2, "auto") == (1920, 1080)
    assert sr_target_size(1920, 1080, 2, "auto") == (3840, 2160)            # the direct route
    assert sr_target_size(48, 32, 4, None) == (192, 128) and sr_target_size(48, 32, 4, (108, 72)) == (108, 72) and sr_target_size(640, 480, 4, 1080) == (1440, 1080)
    with pytest.raises(ValueError, match="320x240.*1280x960.*1440x1080"):
        sr_target_size(320, 240, 4, "auto")                                 # the network gives 960 lines, below 1080
    with pytest.raises(ValueError, match="107x72"):
        sr_target_size(48, 32, 4, (107, 72))
    with pytest.raises(ValueError, match="192x128.*46x32"):
        sr_target_size(48, 32, 4, (46, 32))                                 # below a quarter of the network's output
    for bad in ("big", 0, (1, 2, 3), 1.5):
        with pytest.raises(ValueError):
            sr_target_size(48, 32, 4, bad)


# ------------------------------------------------------------------------------------------------ 5. encode_file
class Reached(Exception):
    pass


def test_encode_file_refusals_before_a_session(tmp_path, monkeypatch):
    from hevc_amd import encoder, sr, yuvio
    from tests.ingest_common import info
    from tests.test_sr_loader import state_dict
    made = []

    def session(cfg, **kw):
        made.append((cfg.width, cfg.height))
        raise Reached()

    monkeypatch.setattr(encoder, "Encoder", session)
    model = sr.load_rrdbnet(state_dict(4, 1))
    out = tmp_path / "o.mp4"
    assert encoder.encode_file(tmp_path / "a.mov", out, info("yuv420p", 48, 32, 3), total_frames=3, sr_target=(108, 72)) == 1          # no model
    assert encoder.encode_file(tmp_path / "a.mov", out, info("yuv420p", 48, 32, 3), total_frames=3, sr_model=model, sr_target=(106, 73)) == 1
    assert encoder.encode_file(tmp_path / "a.mov", out, info("yuv420p", 48, 32, 3), total_frames=3, sr_model=model, sr_target=(400, 300)) == 1       # larger than the network's output
    assert encoder.encode_file(tmp_path / "a.mov", out, info("gbrp", 48, 32, 3), total_frames=3, sr_model=model, sr_target=(40, 32)) == 1            # 4.8 : 1
    for pix in ("yuv422p", "yuv444p10le", "nv12", "p010le", "yuv420p16le"):
        assert encoder.encode_file(tmp_path / "a.mov", out, info(pix, 48, 32, 3), total_frames=3, sr_model=model) == 1, pix
    assert not made
    # a yuv420p source is no longer refused: it reaches the session constructor, at scale x the source and at the target
    frames = [tuple(np.full(s, 100, np.uint8) for s in ((32, 48), (16, 24), (16, 24)))] * 3
    yuvio.write_y4m(tmp_path / "a.y4m", frames, 48, 32)
    with pytest.raises(Reached):
        encoder.encode_file(tmp_path / "a.y4m", out, info("yuv420p", 48, 32, 3), total_frames=3, sr_model=model)
    with pytest.raises(Reached):
        encoder.encode_file(tmp_path / "a.y4m", out, info("yuv420p", 48, 32, 3), total_frames=3, sr_model=model, sr_target=(108, 72))
    assert made == [(192, 128), (108, 72)]


# ------------------------------------------------------------------------------------------------ 6. sanitizers
def test_stepped_kernel_under_address_sanitizer(tmp_path):
    """a stand-alone program (its own main, no python in the process): the stepped kernel over planes and a tensor that end with their last element, and one
    network of each scale.  A read or write past one ends it with the sanitizer's report"""
    exe = tmp_path / "sr_yuv_asan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-w", "-o", str(exe),
                    str(ROOT / "tests" / "emu" / "sr_yuv.cpp"), str(ROOT / "tests" / "sr_yuv_asan_main.cc")], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert p.stdout.strip().endswith("runs")


# ------------------------------------------------------------------------------------------------ 7. the stage entry without a device
def test_stage_entry_validates_first():
    lib = _lib.load()
    y, u, v = Q.source("random", 18, 14, 8)
    out = np.zeros((14, 18, 32), np.uint16)
    no_device = _lib.ENODEV if lib.mihevc_device_count() == 0 else 0

    def call(src, scale=4, planes=(y, u, v), py=18, pc=9):
        return lib.mihevc_k_sr_from_yuv(0, None if src is None else C.byref(src), scale, *[None if p is None else p.ctypes.data for p in planes], py, pc, util.ptr(out))

    assert call(_lib.SrYuv(18, 14, 8, 6, 0)) == no_device
    for bad in (_lib.SrYuv(17, 14, 8, 6, 0), _lib.SrYuv(18, 13, 8, 6, 0), _lib.SrYuv(2, 14, 8, 6, 0), _lib.SrYuv(18, 14, 9, 6, 0), _lib.SrYuv(18, 14, 16, 6, 0),
                _lib.SrYuv(18, 14, 8, 2, 0), _lib.SrYuv(18, 14, 8, 6, 2), None):
        assert call(bad) == _lib.EINVAL, bad
    r = _lib.SrYuv(18, 14, 8, 6, 0)
    r.reserved[1] = 1
    assert call(r) == _lib.EINVAL
    ok = _lib.SrYuv(18, 14, 8, 6, 0)
    assert call(ok, scale=3) == call(ok, py=17) == call(ok, pc=8) == call(ok, planes=(y, None, v)) == _lib.EINVAL
