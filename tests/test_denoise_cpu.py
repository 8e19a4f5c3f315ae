"""CPU: the denoising source (mihevc_send_frame_denoise / mihevc_k_denoise).  The numpy model of tests/denoise_ref.py against hand-worked cases, the
identities of the definition and a sample-by-sample transcription of it; what the model does to a noisy clip; the kernel program of
hevc_amd/csrc/kernels/denoise.h stepped on the CPU (tests/emu/denoise.cpp) against the model, bit for bit, over random initial LDS in the three lane orders; its
division over the whole range; the sanitizer program; the new entry points without a device; the ABI struct; the presets; encode_file(denoise=) in front of a
stand-in ffmpeg."""
import collections
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from hevc_amd import _lib
from tests import denoise_ref as R
from tests import util
from tests.denoise_common import KINDS, SIZES, STRENGTHS, denoise_struct, frames, model, plane_pointers, strength_id
from tests.ingest_common import fake_ffmpeg, info, same_planes      # noqa: F401 (fake_ffmpeg: a fixture)
from tests.test_deint_cpu import StubEncoder

ROOT = Path(__file__).resolve().parents[1]


# ------------------------------------------------------------------------------------------------ 1. the model against hand-worked cases
def scalar_sample(P, C, N, x, y, Ts, Tt, peak):
    """the definition, one sample, Python ints: nothing vectorised, every index written out"""
    H, W = len(C), len(C[0])

    def at(F, r, col):
        return min(int(F[min(max(r, 0), H - 1)][min(max(col, 0), W - 1)]), peak)
    c = at(C, y, x)
    wc = max(Ts, Tt, 1)
    Wsum, acc = wc, wc * c
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                q = at(C, y + dy, x + dx)
                ws = max(0, Ts - abs(q - c))
                Wsum += ws
                acc += ws * q
    for F in (P, N):
        m = 0
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                m += (2 - abs(dy)) * (2 - abs(dx)) * abs(at(F, y + dy, x + dx) - at(C, y + dy, x + dx))
        d = max(abs(at(F, y, x) - c), (m + 8) >> 4)
        wt = max(0, Tt - d)
        Wsum += wt
        acc += wt * at(F, y, x)
    return (acc + (Wsum >> 1)) // Wsum


def test_model_constant_pictures():
    for depth, val in ((8, 0), (8, 255), (8, 77), (10, 1023), (10, 512)):
        p = np.full((16, 24), val, R.dtype(depth))
        for s, t in ((0, 0), (255, 255), (5, 7), (12, 0), (0, 16)):
            assert np.all(R.filter_plane(p, p, p, depth, s, t) == val)


@pytest.mark.parametrize("depth", [8, 10])
def test_model_zero_strengths_are_the_identity(depth):
    """Ts = Tt = 0: wc = 1 and every other weight is 0: out = C (clamped to the depth), whatever P and N hold"""
    P, Cc, N = R.noise_frames(32, 16, depth, 3)
    out, _ = R.denoise(P, Cc, N, depth, (0, 0, 0, 0))
    peak = (1 << depth) - 1
    for o, c in zip(out, Cc):
        assert np.array_equal(o[:c.shape[0], :c.shape[1]], np.minimum(c, peak))
    assert out[0].shape == (16, 32)


@pytest.mark.parametrize("depth", [8, 10])
def test_model_static_clip_without_spatial_strength_is_the_identity(depth):
    """P = N = C and Ts = 0: D = 0 everywhere, so both temporal weights are Tt and all three samples equal C[p]: out = C"""
    _, Cc, _ = R.noise_frames(32, 16, depth, 4, full_word=False)
    for tt in (1, 11, 255):
        out, _ = R.denoise(Cc, Cc, Cc, depth, (0, tt, 0, tt))
        assert all(np.array_equal(o, c) for o, c in zip(out, Cc))


def test_model_keeps_an_isolated_impulse():
    """a flat picture of 50 with one sample of 200 in C only, level 3 (Ts = 8, Tt = 11).  At the impulse every |C[q] - C[p]| and both D are 150: all weights but wc
    are 0, out = 200.  Around it the impulse has ws = 0 and every other contributing sample is 50 (the temporal weight of a neighbour is max(0, 11 - m) with
    m = (150 k + 8) >> 4 = 19 beside it and 9 diagonally): out = 50"""
    Cc = np.full((16, 16), 50, np.uint8)
    Cc[7, 9] = 200
    flat = np.full((16, 16), 50, np.uint8)
    assert np.array_equal(R.filter_plane(flat, Cc, flat, 8, 8, 11), Cc)
    assert (150 * 2 + 8) >> 4 == 19 and (150 + 8) >> 4 == 9


def test_model_three_by_three_by_hand():
    """Ts = 10, Tt = 8, centre of a 3x3 plane.  C: centre 104, seven neighbours 100 (ws = 10 - 4 = 6) and one 115 (ws = max(0, 10 - 11) = 0); wc = 10.
    P = C but 106 at the centre: D_P = 2 there and 0 around, m_P = (4 * 2 + 8) >> 4 = 1, d_P = 2, wt_P = 6.
    N = C + 3 around and 104 at the centre: D_N = 0 there and 3 around, m_N = (3 * 12 + 8) >> 4 = 2 > D_N[p]: d_N = 2, wt_N = 6.
    W = 10 + 7 * 6 + 6 + 6 = 64; acc = 10 * 104 + 42 * 100 + 6 * 106 + 6 * 104 = 6500; out = (6500 + 32) / 64 = 102 (6500 / 64 = 101.56: the rounding term decides)"""
    Cc = np.array([[100, 100, 100], [100, 104, 100], [100, 100, 115]], np.uint8)
    P = Cc.copy()
    P[1, 1] = 106
    N = Cc + 3
    N[1, 1] = 104
    counts = collections.Counter()
    out = R.filter_plane(P, Cc, N, 8, 10, 8, counts)
    assert out[1, 1] == 102 == scalar_sample(P, Cc, N, 1, 1, 10, 8, 255)
    assert 6500 // 64 == 101 and (6500 + 32) // 64 == 102
    assert counts["m_decides"] >= 1


@pytest.mark.parametrize("depth", [8, 10])
def test_model_equals_the_definition_sample_by_sample(depth):
    """a small plane of noise, every sample, the four corners among them: row and column clamps in all three frames"""
    W, H = 18, 8
    P, Cc, N = (f[1][:H, :W] for f in R.noise_frames(2 * W, 2 * H, depth, 5 + depth))
    peak = (1 << depth) - 1
    for s, t in ((255, 255), (12, 0), (0, 16), (5, 7), (90, 200)):
        out = R.filter_plane(P, Cc, N, depth, s, t)
        for y in range(H):
            for x in range(W):
                assert out[y, x] == scalar_sample(P, Cc, N, x, y, s << (depth - 8), t << (depth - 8), peak), (s, t, x, y)


def test_model_bounds_of_the_sums():
    """W <= 11 * 1020 and acc + W / 2 < 2^24: reached by a flat 10-bit picture at peak with every strength 255 (filter_plane asserts both on every call)"""
    p = np.full((16, 16), 1023, np.dtype("<u2"))
    assert np.all(R.filter_plane(p, p, p, 10, 255, 255) == 1023)
    assert 11 * 1020 * 1023 + 11 * 1020 // 2 < 1 << 24


def test_model_fills_the_margin():
    (out, _) = model(SIZES[1], 8, "noise", 2)
    assert out[0].shape == (40, 72) and out[1].shape == (20, 36)
    assert np.all(out[0][:, 70:] == out[0][:, 69:70]) and np.all(out[0][36:] == out[0][35:36]) and np.all(out[2][18:] == out[2][17:18])


def test_inputs_reach_every_weight_class():
    """a condition of the inputs, not a measurement of the kernel: over the inputs and strengths the stepped kernel and the device are compared on, every weight
    class of the model occurs at least 100 times in every plane, at either depth; the non-trivial strengths alone reach all of them too"""
    for depth in (8, 10):
        for pick in (STRENGTHS, STRENGTHS[1:]):
            total = [collections.Counter() for _ in range(3)]
            for size in SIZES:
                for kind in KINDS:
                    for strength in pick:
                        for i, c in enumerate(model(size, depth, kind, strength)[1]):
                            total[i].update(c)
            for i in range(3):
                assert all(total[i][k] >= 100 for k in R.CLASSES), (depth, i, {k: total[i][k] for k in R.CLASSES})


# ------------------------------------------------------------------------------------------------ 2. what the model does to a noisy clip
@pytest.mark.parametrize("speed", [0, 3])
@pytest.mark.parametrize("depth", [8, 10])
def test_model_raises_psnr_against_the_clean_picture(depth, speed):
    """the moving pattern of tests/denoise_ref.py (gradients of at most 3 LSB per sample at 8 bit, below the smallest threshold, under hard checker edges of 127 LSB,
    far above the largest) with noise of sigma 2: at each of levels 1 .. 3 the PSNR of the middle picture against the clean one, over its three planes together
    and over luma alone, is above the input's and does not fall with the level"""
    w, h = 136, 72
    noisy, clean = R.noisy_frames(w, h, depth, 3, speed, seed=5)

    def figures(planes):
        crop = [p[:c.shape[0], :c.shape[1]] for p, c in zip(planes, clean[1])]
        pooled = np.concatenate([np.asarray(p, np.float64).ravel() for p in crop]), np.concatenate([c.ravel() for c in clean[1]])
        return R.psnr(*pooled, depth), R.psnr(crop[0], clean[1][0], depth)
    got = [figures(noisy[1])] + [figures(R.denoise(*noisy, depth, level)[0]) for level in (1, 2, 3)]
    print(f"depth {depth} speed {speed}: PSNR (all planes, luma) of the input and levels 1..3: " + ", ".join(f"{a:.2f}/{b:.2f}" for a, b in got))
    for k in (0, 1):
        assert got[1][k] > got[0][k] and got[2][k] >= got[1][k] and got[3][k] >= got[2][k], got


# ------------------------------------------------------------------------------------------------ 3. the kernel program stepped on the CPU
@pytest.fixture(scope="module")
def emu():
    lib = util.stepped_library()
    lib.emu_denoise.argtypes = [C.POINTER(_lib.Denoise)] + [C.POINTER(C.c_void_p)] * 3 + [C.c_int] * 5 + [C.c_uint] + [C.c_void_p] * 3 + [C.POINTER(C.c_int)]
    lib.emu_denoise_tile.argtypes = [C.POINTER(C.c_int)] * 3
    return lib


def emu_denoise(emu, size, depth, kind, strength, order=0, align=16, seed=1):
    want, _ = model(size, depth, kind, strength)
    out = [np.full(p.shape, 0x77, p.dtype) for p in want]
    stats = (C.c_int * 4)()
    P, Cc, N = frames(size, depth, kind)
    rc = emu.emu_denoise(C.byref(denoise_struct(strength)), plane_pointers(P), plane_pointers(Cc), plane_pointers(N), size[0], size[1], depth, order, align, seed,
                         *[p.ctypes.data for p in out], stats)
    assert rc == 0, rc
    assert stats[0] == 0, f"{stats[0]} misaligned accesses"
    assert stats[1] == 0, f"{stats[1]} samples written outside the coded width"
    assert (stats[2], stats[3]) == (align, align)
    return same_planes(out, want)


def test_sizes_meet_the_tile_edges(emu):
    tw, th, lds = C.c_int(), C.c_int(), C.c_int()
    emu.emu_denoise_tile(C.byref(tw), C.byref(th), C.byref(lds))
    assert 2 * tw.value < 264 < 3 * tw.value and 2 * th.value < 72 < 3 * th.value          # 264x72: two full tiles and a partial one each way
    assert tw.value < 132 < 2 * tw.value and th.value < 36 < 2 * th.value                   # its chroma: one full tile and a partial one each way
    assert 20 < th.value and 16 < th.value and 136 > tw.value                               # 136x20 and 16x16: fewer rows than a tile
    assert R.coded(70) == 72 and R.coded(36) == 40 and (R.coded(70) // 2) % 8 == 4          # 70x36: margin on both axes, a chroma row that ends with half a run
    assert 4 * lds.value <= 160 * 1024                                                      # four workgroups share a CU's 160 KB of LDS


@pytest.mark.parametrize("strength", STRENGTHS, ids=strength_id)
@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_stepped_kernel_equals_model(emu, size, depth, strength):
    for kind in KINDS:
        for order in (0, 1, 2):
            diff = emu_denoise(emu, size, depth, kind, strength, order, 16, seed=17 * order + depth)
            assert not diff, (kind, order, diff)


@pytest.mark.parametrize("align", [1, 4, 8])
@pytest.mark.parametrize("depth", [8, 10])
def test_stepped_kernel_with_misaligned_planes(emu, depth, align):
    for size in SIZES:
        for i, strength in enumerate(STRENGTHS):
            diff = emu_denoise(emu, size, depth, "noise", strength, i % 3, align, seed=align + i)
            assert not diff, (size, strength, diff)


def test_stepped_kernel_clamps_values_above_the_declared_depth():
    assert max(int(p.max()) for f in frames(SIZES[1], 10, "noise") for p in f) > 60000          # what every 10-bit noise case above was fed


def test_stepped_division_is_exact_over_the_whole_range(emu):
    """the reciprocal multiplication with its correction step against integer division: every W up to 11 * 1020, every quotient up to 1023, both ends and the
    middle of each quotient's numerators"""
    assert emu.emu_denoise_div_check() == 0


def test_stepped_kernel_under_address_sanitizer(tmp_path):
    """a stand-alone program (its own main, no python in the process): the stepped kernel over source planes allocated to end with their last sample, every size,
    element type, alignment class and four strengths.  A read past a plane ends it with the sanitizer's report"""
    exe = tmp_path / "denoise_asan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-w", "-o", str(exe),
                    str(ROOT / "tests" / "emu" / "denoise.cpp"), str(ROOT / "tests" / "denoise_asan_main.cc")], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert p.stdout.strip() == "160 runs"


# ------------------------------------------------------------------------------------------------ 4. the entry points without a device
def denoise_call(w=64, h=48, depth=8, **over):
    fr = R.noise_frames(w, h, depth, 1)
    pw, ph = R.coded(w), R.coded(h)
    out = [np.zeros(s, R.dtype(depth)) for s in ((ph, pw), (ph // 2, pw // 2), (ph // 2, pw // 2))]
    a = dict(dn=_lib.denoise_level(2), prev=plane_pointers(fr[0]), cur=plane_pointers(fr[1]), next=plane_pointers(fr[2]), w=w, h=h, pitch_y=w, pitch_c=w // 2, depth=depth,
             oy=out[0].ctypes.data, ou=out[1].ctypes.data, ov=out[2].ctypes.data)
    a.update(over)
    rc = _lib.load().mihevc_k_denoise(0, None if a["dn"] is None else C.byref(a["dn"]), a["prev"], a["cur"], a["next"], a["w"], a["h"], a["pitch_y"], a["pitch_c"],
                                      a["depth"], a["oy"], a["ou"], a["ov"])
    del fr, out
    return rc


def test_denoise_rejects_bad_arguments():
    for w, h in ((63, 48), (64, 47), (14, 48), (64, 14)):      # odd, too small
        assert denoise_call(w=w, h=h, pitch_y=64, pitch_c=32) == _lib.EINVAL, (w, h)
    assert denoise_call(pitch_y=63) == _lib.EINVAL and denoise_call(pitch_c=31) == _lib.EINVAL
    for depth in (9, 12, 16, 0):
        assert denoise_call(depth=depth) == _lib.EINVAL
    assert denoise_call(dn=None) == _lib.EINVAL
    for k in range(4):
        for bad in (-1, 256, 1 << 20):
            t = [5, 7, 5, 7]
            t[k] = bad
            assert denoise_call(dn=_lib.Denoise(*t)) == _lib.EINVAL, t
        dn = _lib.denoise_level(1)
        dn.reserved[k] = 1
        assert denoise_call(dn=dn) == _lib.EINVAL
    for k in ("prev", "cur", "next", "oy", "ou", "ov"):
        assert denoise_call(**{k: None}) == _lib.EINVAL, k
    y = np.zeros((48, 64), np.uint8)
    for k in ("prev", "cur", "next"):
        assert denoise_call(**{k: (C.c_void_p * 3)(y.ctypes.data, None, y.ctypes.data)}) == _lib.EINVAL, k


def test_send_frame_denoise_rejects_a_null_session():
    y = np.zeros((48, 64), np.uint8)
    assert _lib.load().mihevc_send_frame_denoise(None, C.byref(_lib.denoise_level(2)), y.ctypes.data, y.ctypes.data, y.ctypes.data, 64, 32, 0, 0) == _lib.EINVAL


@pytest.mark.skipif(_lib.load().mihevc_device_count() > 0, reason="a GPU is present")
def test_no_gpu_means_loud_failure():
    assert denoise_call() == _lib.ENODEV and denoise_call(depth=10, h=50) == _lib.ENODEV          # (a height that is no multiple of 4 is fine here)
    assert denoise_call(dn=_lib.Denoise(256, 0, 0, 0)) == _lib.EINVAL          # the arguments are judged first


def test_denoise_layout_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mihevc.h"\nint main(void){printf("%zu %zu %zu %zu %zu\\n",'
                   "sizeof(mihevc_denoise),offsetof(mihevc_denoise,luma_temporal),offsetof(mihevc_denoise,chroma_spatial),"
                   "offsetof(mihevc_denoise,chroma_temporal),offsetof(mihevc_denoise,reserved));return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    D = _lib.Denoise
    assert got == [C.sizeof(D), D.luma_temporal.offset, D.chroma_spatial.offset, D.chroma_temporal.offset, D.reserved.offset] and got == [32, 4, 8, 12, 16]
    assert _lib.load().mihevc_abi_version() == 6
    assert {"mihevc_send_frame_denoise", "mihevc_k_denoise"} <= set(_lib.EXPORTS)


def test_levels():
    assert [tuple(getattr(_lib.denoise_level(n), f) for f in ("luma_spatial", "luma_temporal", "chroma_spatial", "chroma_temporal")) for n in range(4)] == list(R.LEVELS)
    assert R.LEVELS[0] == (0, 0, 0, 0) and all(a <= b for lo, hi in zip(R.LEVELS, R.LEVELS[1:]) for a, b in zip(lo, hi))
    for bad in (-1, 4, 2.0, "2", None, True):
        with pytest.raises(ValueError):
            _lib.denoise_level(bad)


# ------------------------------------------------------------------------------------------------ 5. encode_file(denoise=)
class DenoiseStub(StubEncoder):
    def send_denoise(self, y, u, v, strength=2, asynchronous=False, pts=None):
        s = strength if not isinstance(strength, _lib.Denoise) else (strength.luma_spatial, strength.luma_temporal, strength.chroma_spatial, strength.chroma_temporal)
        self.calls.append(("denoise", y.shape, u.shape, str(y.dtype), s, pts))
        self.sent += 1


def test_encode_file_denoise_in_front_of_the_pipe(fake_ffmpeg, tmp_path, monkeypatch):
    from hevc_amd import encoder
    w, h, n = 64, 48, 3
    monkeypatch.setenv("FAKE_FRAMES", str(n))
    monkeypatch.setenv("FAKE_FB", str(w * h * 3 // 2))
    monkeypatch.setattr(encoder, "Encoder", DenoiseStub)

    def run(out, pix="yuv420p", **kw):
        StubEncoder.made.clear()
        rc = encoder.encode_file(tmp_path / "a.mov", tmp_path / out, info(pix, w, h, n), total_frames=n, **kw)
        return rc, (StubEncoder.made[0] if StubEncoder.made else None)

    # a level: its preset with every frame; the pipe is asked for the frames as they are, no filter in front
    for level in (1, 2, 3):
        rc, enc = run("f.mp4", denoise=level)
        argv = fake_ffmpeg.read_text().split("\n")[-2].split()
        assert rc == 0 and not {"-vf", "-filter:v"} & set(argv) and not any("hqdn3d" in a or "nlmeans" in a for a in argv)
        assert enc.calls == [("denoise", (h, w), (h // 2, w // 2), "uint8", R.LEVELS[level], i) for i in range(n)]
    # four thresholds of one's own
    rc, enc = run("g.mp4", denoise=(12, 0, 0, 16))
    assert rc == 0 and enc.calls == [("denoise", (h, w), (h // 2, w // 2), "uint8", (12, 0, 0, 16), i) for i in range(n)]
    # None and 0: as before
    for kw in ({}, dict(denoise=None), dict(denoise=0)):
        rc, enc = run("h.mp4", **kw)
        assert rc == 0 and enc.calls == [("plain", (h, w), i) for i in range(n)], kw
    # refused: together with the other sources, several devices, a level or thresholds out of range, another layout
    for kw in (dict(deinterlace="frame"), dict(size=(32, 24)), dict(native_rgb=True), dict(devices=[0, 1]), dict(devices=[0, 1], row_split=True), dict(denoise=4),
               dict(denoise=-1), dict(denoise=(1, 2, 3)), dict(denoise=(1, 2, 3, 256)), dict(denoise="2")):
        rc, enc = run("m.mp4", **{"denoise": 2, **kw})
        assert rc == 1 and (enc is None or not enc.calls), kw
    monkeypatch.setenv("FAKE_FB", str(w * h * 2))
    rc, enc = run("l.mp4", pix="yuv422p", denoise=2)
    assert rc == 1 and (enc is None or not enc.calls)
