"""CPU: the deinterlacing source (mihevc_send_frame_deint / mihevc_k_deinterlace).  The numpy model of tests/deint_ref.py against hand-worked cases and
a sample-by-sample transcription of the definition; the kernel program of hevc_amd/csrc/kernels/deint.h stepped on the CPU (tests/emu/deint.cpp) against the
model, bit for bit, over random initial LDS in the three lane orders; the sanitizer program; the new entry points without a device; the ABI struct; the y4m
interlace tag; encode_file(deinterlace=) in front of a stand-in ffmpeg and ffprobe."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from hevc_amd import _lib
from tests import deint_ref as R
from tests import util
from tests.deint_common import COMBOS, KINDS, SIZES, frames, model, plane_pointers
from tests.ingest_common import fake_ffmpeg, info, same_planes      # noqa: F401 (fake_ffmpeg: a fixture)

ROOT = Path(__file__).resolve().parents[1]


# ------------------------------------------------------------------------------------------------ 1. the model against hand-worked cases
def scalar_sample(P, C, N, x, y, second, peak):
    """the definition, one sample, Python ints: nothing vectorised, every index written out"""
    H, W = len(C), len(C[0])

    def at(F, r, col):
        r = r + 2 if r < 0 else r - 2 if r >= H else r
        return min(int(F[r][min(max(col, 0), W - 1)]), peak)
    A, Z = (C, N) if second else (P, C)
    c, e, d = at(C, y - 1, x), at(C, y + 1, x), (at(A, y, x) + at(Z, y, x)) >> 1
    t0 = abs(at(A, y, x) - at(Z, y, x))
    t1 = (abs(at(P, y - 1, x) - c) + abs(at(P, y + 1, x) - e)) >> 1
    t2 = (abs(at(N, y - 1, x) - c) + abs(at(N, y + 1, x) - e)) >> 1
    diff = max(t0 >> 1, t1, t2)

    def score(j):
        return sum(abs(at(C, y - 1, x + k + j) - at(C, y + 1, x + k - j)) for k in (-1, 0, 1))

    def pred(j):
        return (at(C, y - 1, x + j) + at(C, y + 1, x - j)) >> 1
    best, sp = score(0) - 1, pred(0)
    for s in (-1, 1):
        if score(s) < best:
            best, sp = score(s), pred(s)
            if score(2 * s) < best:
                best, sp = score(2 * s), pred(2 * s)
    b, f = (at(A, y - 2, x) + at(Z, y - 2, x)) >> 1, (at(A, y + 2, x) + at(Z, y + 2, x)) >> 1
    mx = max(d - e, d - c, min(b - c, f - e))
    mn = min(d - e, d - c, max(b - c, f - e))
    diff = max(diff, mn, -mx)
    return d + diff if sp > d + diff else d - diff if sp < d - diff else sp


def test_model_flat_plane():
    for depth, val in ((8, 0), (8, 255), (8, 77), (10, 1023), (10, 512)):
        p = np.full((16, 24), val, R.dtype(depth))
        for keep, second in COMBOS:
            assert np.all(R.filter_plane(p, p, p, depth, keep, second) == val)


def test_model_static_clip_weaves():
    """P = C = N, a vertical ramp of 10 per row: t0 = t1 = t2 = 0; inside the plane b - c = -10 and f - e = 10, so mn = -10, mx = 10, diff stays 0 and the missing
    row is d = C[y] itself, whatever the columns hold.  Row 0 (keep = 1): c = e = C[1], b = C[0] (row -2 -> 0), f = C[2]: d - e = d - c = b - c = -10, f - e = 10:
    mx = -10, mn = -10, diff = max(0, -10, 10) = 10, sp = C[1] = d + 10: out = C[1].  Row H - 1 (keep = 0): mirrored, out = C[H - 2]"""
    H, W = 16, 20
    col = np.random.default_rng(1).integers(0, 60, W)
    C0 = (10 * np.arange(H)[:, None] + col[None, :]).astype(np.uint8)
    for keep, second in COMBOS:
        out = R.filter_plane(C0, C0, C0, 8, keep, second)
        assert np.array_equal(out[2:H - 2], C0[2:H - 2])
    flat_cols = (10 * np.arange(H)[:, None] + np.zeros((1, W), int)).astype(np.uint8)
    assert np.all(R.filter_plane(flat_cols, flat_cols, flat_cols, 8, 1, 0)[0] == 10)
    assert np.all(R.filter_plane(flat_cols, flat_cols, flat_cols, 8, 0, 0)[H - 1] == 10 * (H - 2))


@pytest.mark.parametrize("j", [-2, -1, 0, 1, 2])
def test_model_follows_a_diagonal_edge(j):
    """C[2] steps from 0 to V at column p, C[4] at column q = p - 2 j; the missing row 3 holds V / 2.  With the step thresholds written out (score(i) counts the
    k in {-1, 0, 1} that lie between p - i - x and q + i - x): at x = (p + q) / 2 offset j has score 0 and wins through the chain the definition prescribes
    (j = 2: score(0) = 3 V, score(-1) = 3 V, score(1) = 2 V < 3 V - 1, score(2) = 0), and pred(j) = (C[2][x + j] + C[4][x - j]) >> 1 = V, where pred(0) would give
    V / 2 (j = 0: both steps at p, x = p: V either way).  P and N differ from C by V on rows 2 and 4, so t1 = t2 = V and the clamp leaves sp alone"""
    V, W, H, p = 200, 24, 8, 12
    q = p - 2 * j
    Cc = np.full((H, W), V // 2, np.uint8)
    Cc[2] = np.where(np.arange(W) >= p, V, 0)
    Cc[4] = np.where(np.arange(W) >= q, V, 0)
    Pp = Cc.copy()
    Pp[2], Pp[4] = V - Cc[2], V - Cc[4]
    x = (p + q) // 2
    counts = R.collections.Counter()
    out = R.filter_plane(Pp, Cc, Pp, 8, 0, 0, counts)
    assert out[3, x] == V == scalar_sample(Pp, Cc, Pp, x, 3, 0, 255)
    assert counts[f"offset{j:+d}"] > 0
    if j:
        assert (int(Cc[2, x]) + int(Cc[4, x])) >> 1 == V // 2          # what the vertical average would have given


def test_model_clamps_both_ways():
    """a static clip whose rows y - 2 .. y + 2 are V, V, 0, V, V: sp = V, d = 0, b = f = V: mx = max(-V, -V, min(0, 0)) = 0, mn = -V, diff = 0: out = d = 0, clamped from
    above (a dark line one row high survives).  Inverted: out = V, clamped from below"""
    V = 180
    for line, other, name in ((0, V, "clamp_high"), (V, 0, "clamp_low")):
        Cc = np.full((12, 16), other, np.uint8)
        Cc[5] = line
        counts = R.collections.Counter()
        out = R.filter_plane(Cc, Cc, Cc, 8, 0, 0, counts)
        assert np.all(out[5] == line) and counts[name] >= 16
        assert scalar_sample(Cc, Cc, Cc, 7, 5, 0, 255) == line


@pytest.mark.parametrize("depth", [8, 10])
def test_model_equals_the_definition_sample_by_sample(depth):
    """a small plane of noise, every sample, the four corners among them: column clamp at x = 0 and W - 1, row replacement at y = 0, 1, H - 2, H - 1, both keep"""
    W, H = 18, 8
    P, Cc, N = (f[1][:H, :W] for f in R.noise_frames(2 * W, 2 * H, depth, 5 + depth))
    peak = (1 << depth) - 1
    for keep, second in COMBOS:
        out = R.filter_plane(P, Cc, N, depth, keep, second)
        for y in range(H):
            for x in range(W):
                want = min(int(Cc[y][x]), peak) if (y & 1) == keep else scalar_sample(P, Cc, N, x, y, second, peak)
                assert out[y, x] == want, (keep, second, x, y)


def test_model_fills_the_margin():
    (out, _) = model(SIZES[0], 8, "noise", 1, 1)
    assert out[0].shape == (40, 72) and out[1].shape == (20, 36)
    assert np.all(out[0][:, 70:] == out[0][:, 69:70]) and np.all(out[0][36:] == out[0][35:36]) and np.all(out[2][18:] == out[2][17:18])


@pytest.mark.parametrize("keep,second", COMBOS)
def test_inputs_reach_every_branch(keep, second):
    """a condition of the inputs, not a measurement of the kernel: on the noise and on the woven clip every branch counter of the model is non-zero"""
    for kind in KINDS:
        for depth in (8, 10):
            _, counts = model(SIZES[0], depth, kind, keep, second)
            assert all(counts[b] > 0 for b in R.BRANCHES), (kind, depth, {b: counts[b] for b in R.BRANCHES})


# ------------------------------------------------------------------------------------------------ 2. the kernel program stepped on the CPU
@pytest.fixture(scope="module")
def emu():
    lib = util.stepped_library()
    lib.emu_deint.argtypes = [C.POINTER(C.c_void_p)] * 3 + [C.c_int] * 7 + [C.c_uint] + [C.c_void_p] * 3 + [C.POINTER(C.c_int)]
    lib.emu_deint_tile.argtypes = [C.POINTER(C.c_int)] * 3
    return lib


def emu_deint(emu, size, depth, kind, keep, second, order=0, align=16, seed=1):
    want, _ = model(size, depth, kind, keep, second)
    out = [np.full(p.shape, 0x77, p.dtype) for p in want]
    stats = (C.c_int * 4)()
    P, Cc, N = frames(size, depth, kind)
    rc = emu.emu_deint(plane_pointers(P), plane_pointers(Cc), plane_pointers(N), size[0], size[1], depth, keep, second, order, align, seed,
                       *[p.ctypes.data for p in out], stats)
    assert rc == 0, rc
    assert stats[0] == 0, f"{stats[0]} misaligned accesses"
    assert stats[1] == 0, f"{stats[1]} samples written outside the coded width"
    assert (stats[2], stats[3]) == (align, align)
    return same_planes(out, want)


def test_sizes_meet_the_tile_edges(emu):
    tw, th, lds = C.c_int(), C.c_int(), C.c_int()
    emu.emu_deint_tile(C.byref(tw), C.byref(th), C.byref(lds))
    assert 136 > tw.value and 136 % tw.value and 72 > th.value and 72 % th.value          # 136x72: more than one tile each way, partial tiles
    assert 68 < tw.value and 36 > th.value                                                  # its chroma: one tile across, two down
    assert 20 < th.value and 264 > 2 * tw.value                                             # 264x20: fewer rows than a tile
    assert R.coded(70) == 72 and R.coded(36) == 40 and (R.coded(70) // 2) % 8 == 4          # 70x36: margin on both axes, a chroma row that ends with half a run
    assert 4 * lds.value <= 160 * 1024                                                      # four workgroups share a CU's 160 KB of LDS


@pytest.mark.parametrize("keep,second", COMBOS)
@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_stepped_kernel_equals_model(emu, size, depth, keep, second):
    for kind in KINDS:
        for order in (0, 1, 2):
            diff = emu_deint(emu, size, depth, kind, keep, second, order, 16, seed=17 * order + depth)
            assert not diff, (kind, order, diff)


@pytest.mark.parametrize("align", [1, 4, 8])
@pytest.mark.parametrize("depth", [8, 10])
def test_stepped_kernel_with_misaligned_planes(emu, depth, align):
    for size in SIZES:
        for i, (keep, second) in enumerate(COMBOS):
            diff = emu_deint(emu, size, depth, "noise", keep, second, i % 3, align, seed=align + i)
            assert not diff, (size, keep, second, diff)


def test_stepped_kernel_clamps_values_above_the_declared_depth():
    assert max(int(p.max()) for f in frames(SIZES[0], 10, "noise") for p in f) > 60000          # what every 10-bit noise case above was fed


def test_stepped_kernel_under_address_sanitizer(tmp_path):
    """a stand-alone program (its own main, no python in the process): the stepped kernel over source planes allocated to end with their last sample, every size,
    element type, alignment class and keep x second.  A read past a plane ends it with the sanitizer's report"""
    exe = tmp_path / "deint_asan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-w", "-o", str(exe),
                    str(ROOT / "tests" / "emu" / "deint.cpp"), str(ROOT / "tests" / "deint_asan_main.cc")], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert p.stdout.strip() == "160 runs"


# ------------------------------------------------------------------------------------------------ 3. the entry points without a device
def deint_call(w=64, h=48, depth=8, keep=0, second=0, **over):
    fr = R.noise_frames(w, h, depth, 1)
    pw, ph = R.coded(w), R.coded(h)
    out = [np.zeros(s, R.dtype(depth)) for s in ((ph, pw), (ph // 2, pw // 2), (ph // 2, pw // 2))]
    a = dict(prev=plane_pointers(fr[0]), cur=plane_pointers(fr[1]), next=plane_pointers(fr[2]), w=w, h=h, pitch_y=w, pitch_c=w // 2, depth=depth, keep=keep, second=second,
             oy=out[0].ctypes.data, ou=out[1].ctypes.data, ov=out[2].ctypes.data)
    a.update(over)
    rc = _lib.load().mihevc_k_deinterlace(0, a["prev"], a["cur"], a["next"], a["w"], a["h"], a["pitch_y"], a["pitch_c"], a["depth"], a["keep"], a["second"],
                                          a["oy"], a["ou"], a["ov"])
    del fr, out
    return rc


def test_deinterlace_rejects_bad_arguments():
    for w, h in ((63, 48), (64, 46), (64, 50), (14, 48), (64, 12)):      # odd width, heights that are no multiple of 4, too small
        assert deint_call(w=w, h=h, pitch_y=64, pitch_c=32) == _lib.EINVAL, (w, h)
    assert deint_call(pitch_y=63) == _lib.EINVAL and deint_call(pitch_c=31) == _lib.EINVAL
    for depth in (9, 12, 16, 0):
        assert deint_call(depth=depth) == _lib.EINVAL
    for k in ("keep", "second"):
        assert deint_call(**{k: 2}) == _lib.EINVAL and deint_call(**{k: -1}) == _lib.EINVAL
    for k in ("prev", "cur", "next", "oy", "ou", "ov"):
        assert deint_call(**{k: None}) == _lib.EINVAL, k
    y = np.zeros((48, 64), np.uint8)
    for k in ("prev", "cur", "next"):
        assert deint_call(**{k: (C.c_void_p * 3)(y.ctypes.data, None, y.ctypes.data)}) == _lib.EINVAL, k


def test_send_frame_deint_rejects_a_null_session():
    y = np.zeros((48, 64), np.uint8)
    assert _lib.load().mihevc_send_frame_deint(None, C.byref(_lib.Deint(1, 0)), y.ctypes.data, y.ctypes.data, y.ctypes.data, 64, 32, 0, 0) == _lib.EINVAL


@pytest.mark.skipif(_lib.load().mihevc_device_count() > 0, reason="a GPU is present")
def test_no_gpu_means_loud_failure():
    assert deint_call() == _lib.ENODEV and deint_call(depth=10, keep=1, second=1) == _lib.ENODEV
    assert deint_call(keep=2) == _lib.EINVAL          # the arguments are judged first


def test_deint_layout_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mihevc.h"\nint main(void){printf("%zu %zu %zu\\n",'
                   "sizeof(mihevc_deint),offsetof(mihevc_deint,field_rate),offsetof(mihevc_deint,reserved));return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(_lib.Deint), _lib.Deint.field_rate.offset, _lib.Deint.reserved.offset] and got[0] == 32
    assert _lib.load().mihevc_abi_version() == 6
    assert {"mihevc_send_frame_deint", "mihevc_k_deinterlace"} <= set(_lib.EXPORTS)


# ------------------------------------------------------------------------------------------------ 4. yuvio and probe
def test_y4m_interlace_tag_round_trip(tmp_path):
    from hevc_amd import yuvio
    fr = [tuple(p for p in f) for f in R.woven_frames(32, 16, 8, 2)]
    yuvio.write_y4m(tmp_path / "p.y4m", fr, 32, 16, fps=25)
    assert (tmp_path / "p.y4m").read_bytes().startswith(b"YUV4MPEG2 W32 H16 F25:1 Ip A1:1 C420jpeg\n")          # the default header: byte for byte as before
    assert yuvio.open_clip(tmp_path / "p.y4m").interlace == "p"
    for tag in ("t", "b"):
        yuvio.write_y4m(tmp_path / f"{tag}.y4m", fr, 32, 16, fps=25, interlace=tag)
        clip = yuvio.open_clip(tmp_path / f"{tag}.y4m")
        assert clip.interlace == tag and clip.n_frames == 2
        got = list(clip.frames())
        clip.close()
        assert all(np.array_equal(a, b) for g, f in zip(got, fr) for a, b in zip(g, f))
    with pytest.raises(ValueError):
        yuvio.write_y4m(tmp_path / "x.y4m", fr, 32, 16, interlace="x")


def test_field_order_names():
    from hevc_amd import probe
    assert [probe.top_field_first_of(s) for s in ("tt", "tb", "bb", "bt", "progressive", "unknown", "", None)] == [True, True, False, False, None, None, None, None]


# ------------------------------------------------------------------------------------------------ 5. encode_file(deinterlace=)
class StubEncoder:
    """stands where the session would: keeps what encode_file hands it"""
    made = []

    def __init__(self, cfg, device=0):
        self.cfg, self.calls, self.sent = cfg, [], 0
        StubEncoder.made.append(self)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass

    def send_deint(self, y, u, v, tff=True, field_rate=False, asynchronous=False, pts=None):
        self.calls.append(("deint", y.shape, u.shape, str(y.dtype), tff, field_rate, pts))
        self.sent += 2 if field_rate else 1

    def send(self, y, u, v, pts=None):
        self.calls.append(("plain", y.shape, pts))
        self.sent += 1

    def packets_dts(self):
        while self.sent > getattr(self, "out", 0):
            self.out = getattr(self, "out", 0) + 1
            yield b"\x00\x00\x00\x01\x26\x01" + bytes(8), self.out - 1, self.out == 1, self.out - 1

    def flush(self):
        pass

    def headers(self):
        buf = (C.c_uint8 * 4096)()
        n = _lib.load().mihevc_write_parameter_sets(C.byref(self.cfg), buf, 4096)
        assert n > 0
        return bytes(buf[:n])


@pytest.fixture
def fake_ffprobe(fake_ffmpeg, tmp_path):
    """a stand-in ffprobe beside the stand-in ffmpeg: prints one video stream with the field_order of $FAKE_FIELD_ORDER"""
    f = tmp_path / "bin" / "ffprobe"
    f.write_text('#!/bin/sh\nprintf \'{"streams":[{"codec_type":"audio"},{"codec_type":"video","field_order":"%s"}]}\' "$FAKE_FIELD_ORDER"\n')
    f.chmod(0o755)
    return f


def test_encode_file_deinterlace_in_front_of_the_pipe(fake_ffprobe, fake_ffmpeg, tmp_path, monkeypatch):
    from hevc_amd import encoder, mp4
    w, h, n = 64, 48, 3
    monkeypatch.setenv("FAKE_FRAMES", str(n))
    monkeypatch.setenv("FAKE_FB", str(w * h * 3 // 2))
    monkeypatch.setattr(encoder, "Encoder", StubEncoder)

    def run(out, pix="yuv420p", **kw):
        StubEncoder.made.clear()
        rc = encoder.encode_file(tmp_path / "a.mov", tmp_path / out, info(pix, w, h, n), total_frames=n, **kw)
        return rc, (StubEncoder.made[0] if StubEncoder.made else None)

    # 'frame': one call per frame, the rate as probed; the pipe is asked for the frames as they are, no filter in front
    monkeypatch.setenv("FAKE_FIELD_ORDER", "tt")
    rc, enc = run("f.mp4", deinterlace="frame")
    argv = fake_ffmpeg.read_text().split("\n")[-2].split()
    assert rc == 0 and not {"-vf", "-filter:v"} & set(argv) and not any("yadif" in a for a in argv)
    assert enc.calls == [("deint", (h, w), (h // 2, w // 2), "uint8", True, False, i) for i in range(n)]
    assert (enc.cfg.fps_num, enc.cfg.fps_den) == (30, 1)
    # 'field': twice the rate in the session, its level and the track; pts in field periods
    monkeypatch.setenv("FAKE_FIELD_ORDER", "bb")
    rc, enc = run("g.mp4", deinterlace="field")
    assert rc == 0 and enc.calls == [("deint", (h, w), (h // 2, w // 2), "uint8", False, True, 2 * i) for i in range(n)]
    assert (enc.cfg.fps_num, enc.cfg.fps_den) == (60, 1)
    from hevc_amd.transcoder import calculate_apple_hevc_level
    fast = info("yuv420p", w, h, 2 * n)
    fast.fps = 60.0
    assert enc.cfg.level_idc == int(round(float(calculate_apple_hevc_level(fast)[0]) * 30))
    data = (tmp_path / "g.mp4").read_bytes()
    start, end = 0, len(data)
    for name in ("moov", "trak", "mdia", "minf", "stbl", "stsz"):
        _, start, end = [b for b in mp4.parse_boxes(data, start, end) if b[0] == name][0]
    assert int.from_bytes(data[start + 8:start + 12], "big") == 2 * n
    # tff= outranks the probe
    rc, enc = run("h.mp4", deinterlace="frame", tff=True)
    assert rc == 0 and all(c[4] is True for c in enc.calls)
    # 'auto': the probe's word; bt is bottom first, tb top first, anything else is progressive and nothing changes
    for order, want in (("bt", False), ("tb", True)):
        monkeypatch.setenv("FAKE_FIELD_ORDER", order)
        rc, enc = run("i.mp4", deinterlace="auto")
        assert rc == 0 and [c[0] for c in enc.calls] == ["deint"] * n and all(c[4] is want and c[5] is False for c in enc.calls)
    for order in ("progressive", "unknown", ""):
        monkeypatch.setenv("FAKE_FIELD_ORDER", order)
        rc, enc = run("j.mp4", deinterlace="auto")
        assert rc == 0 and enc.calls == [("plain", (h, w), i) for i in range(n)]
    # without the option: as before
    rc, enc = run("k.mp4")
    assert rc == 0 and enc.calls == [("plain", (h, w), i) for i in range(n)]
    # refused: another layout, size=, native_rgb, an unknown mode, a height that is no multiple of 4
    monkeypatch.setenv("FAKE_FIELD_ORDER", "tt")
    monkeypatch.setenv("FAKE_FB", str(w * h * 2))
    rc, enc = run("l.mp4", pix="yuv422p", deinterlace="frame")
    assert rc == 1 and (enc is None or not enc.calls)
    monkeypatch.setenv("FAKE_FB", str(w * h * 3 // 2))
    for kw in (dict(size=(32, 24)), dict(native_rgb=True), dict(deinterlace="bob")):
        rc, enc = run("m.mp4", **{"deinterlace": "frame", **kw})
        assert rc == 1 and (enc is None or not enc.calls), kw
    StubEncoder.made.clear()
    monkeypatch.setenv("FAKE_FB", str(w * 46 * 3 // 2))
    assert encoder.encode_file(tmp_path / "a.mov", tmp_path / "n.mp4", info("yuv420p", w, 46, n), total_frames=n, deinterlace="frame") == 1


def test_encode_file_auto_takes_the_y4m_tag(tmp_path, monkeypatch):
    from hevc_amd import encoder, probe, yuvio
    w, h, n = 64, 48, 3
    monkeypatch.setattr(encoder, "Encoder", StubEncoder)
    fr = R.woven_frames(w, h, 8, n)
    for tag, want in (("t", True), ("b", False), ("p", None)):
        StubEncoder.made.clear()
        yuvio.write_y4m(tmp_path / f"{tag}.y4m", fr, w, h, fps=25, interlace=tag)
        nfo = probe.VideoInfo(w, h, 25.0, "bt709", "bt709", "bt709", "yuv420p", "", "", 0, False, "eng", n, n / 25.0)
        assert encoder.encode_file(tmp_path / f"{tag}.y4m", tmp_path / f"{tag}.mp4", nfo, total_frames=n, deinterlace="auto") == 0
        (enc,) = StubEncoder.made
        if want is None:
            assert enc.calls == [("plain", (h, w), i) for i in range(n)]
        else:
            assert enc.calls == [("deint", (h, w), (h // 2, w // 2), "uint8", want, False, i) for i in range(n)]
