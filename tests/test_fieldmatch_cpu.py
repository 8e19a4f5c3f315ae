"""CPU (-m "not gpu"): inverse telecine.  The numpy model of tests/fieldmatch_ref.py against the definition sample by sample; the recovery
property on the model pipeline (a clean telecined clip comes back as exactly its film frames, and every later cycle drops exactly its repeat); the programs of
hevc_amd/csrc/kernels/fieldmatch.h stepped on the CPU against the model bit for bit, also under AddressSanitizer in a stand-alone program; the planner of
hevc_amd/csrc/fieldmatch_plan.h against a Python restatement; the entry points without a device; the struct layouts."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from hevc_amd import _lib
from tests import deint_ref as D
from tests import fieldmatch_ref as R
from tests import util
from tests.deint_common import plane_pointers
from tests.fieldmatch_common import H, SIZES, W, expected_film, film, frames, hybrid, model_metrics, telecined
from tests.ingest_common import same_planes

ROOT = Path(__file__).resolve().parents[1]
PHASES = range(5)
ORDERS = [(stored, declared) for stored in (True, False) for declared in (True, False)]


# ------------------------------------------------------------------------------------------------ 1. the model and the clips
@pytest.mark.parametrize("depth", [8, 10])
def test_model_equals_the_definition_sample_by_sample(depth):
    for kind, size in (("noise", (34, 36)), ("film", (70, 36))):
        P, Cc, N = (f[0][:, :size[0]] for f in frames((70, 36), depth, kind))
        for keep in (0, 1):
            got = R.metrics(P, Cc, N, depth, keep)
            assert got == R.scalar_metrics(P, Cc, N, depth, keep), (kind, keep)
            assert kind == "film" or min(got) > 0          # noise: every number is exercised


@pytest.mark.parametrize("depth", [8, 10])
def test_film_frames_have_no_combed_sample_and_differ(depth):
    fl = film(depth, 12)
    for a, b in zip(fl, fl[1:]):
        for keep in (0, 1):
            m = R.metrics(a[0], b[0], b[0], depth, keep)          # P = a, C = b: the c candidate is film frame b itself
            assert m[0] == 0 and m[3] == 0, "a film frame has a combed sample"
            assert m[7] > 0 and m[6] > 0, "consecutive film frames do not differ"
            assert m[1] > 0 and m[4] > 0, "fields of neighbouring film frames weave without a comb: the clips could not tell a wrong match"


def run_model(clip, depth, declared_tff, decimate, deint=True):
    return R.pictures(list(clip), depth, declared_tff, decimate, deint)


@pytest.mark.parametrize("stored,declared", ORDERS, ids=lambda v: "tff" if v else "bff")
@pytest.mark.parametrize("phase", PHASES)
def test_recovery_of_every_frame_that_has_its_neighbour(phase, stored, declared):
    depth, n = 8, 12
    clip, src = telecined(depth, n, phase, stored)
    fl = film(depth, max(b for _, b in src) + 1)
    pics, decided = run_model(clip, depth, declared, False)
    want = expected_film(src, declared, stored)
    assert sum(where is not None for _, where in want) >= n - 2
    assert {where for _, where in want if where} >= ({"c", "p"} if stored == declared else {"c", "n"})
    for k, ((f, where), (pts, planes), d) in enumerate(zip(want, pics, decided)):
        assert pts == k
        if where is None:          # (an orphan field at the clip's edge: the least combed weave, or the deinterlacer's picture)
            continue
        assert not d["deinterlaced"] and d["metrics"]["cpn".index(where)] == 0
        diff = same_planes(planes, R.weave(fl[f], fl[f], depth, 0))
        assert not diff, (k, where, d["match"], diff)


@pytest.mark.parametrize("stored,declared", ORDERS, ids=lambda v: "tff" if v else "bff")
@pytest.mark.parametrize("phase", PHASES)
def test_every_cycle_after_the_first_drops_exactly_its_repeat(phase, stored, declared):
    depth, n = 8, 15
    clip, src = telecined(depth, n, phase, stored)
    want = expected_film(src, declared, stored)
    pics, decided = run_model(clip, depth, declared, True)
    assert len(pics) == 12 and [p for p, _ in pics] == list(range(12))
    for k0 in (5, 10):
        repeats = [k for k in range(k0, k0 + 5) if want[k][0] == want[k - 1][0]]
        assert len(repeats) == 1
        assert [k for k in range(k0, k0 + 5) if decided[k]["dropped"]] == repeats
        assert decided[repeats[0]]["metrics"][6:] == [0, 0]
    assert sum(d["dropped"] for d in decided[:5]) == 1 and not decided[0]["dropped"]


@pytest.mark.parametrize("depth", [8, 10])
def test_a_ten_frame_clip_that_starts_clean_yields_its_eight_film_frames(depth):
    clip, src = telecined(depth, 10, 0)
    fl = film(depth, 8)
    assert src[0] == (0, 0) and src[-1] == (7, 7)
    pics, decided = run_model(clip, depth, True, True)
    assert [d["dropped"] for d in decided] == [False, False, True, False, False] * 2
    assert [p for p, _ in pics] == list(range(8))
    for (pts, planes), f in zip(pics, fl):
        assert not same_planes(planes, R.weave(f, f, depth, 0)), pts


def test_noise_does_not_change_the_decisions():
    for phase in PHASES:
        clip, src = telecined(8, 15, phase)
        clean = run_model(clip, 8, True, True)[1]
        noisy = run_model(telecined(8, 15, phase, True, noise=2)[0], 8, True, True)[1]
        for k, (a, b, (_, where)) in enumerate(zip(clean, noisy, expected_film(src, True, True))):
            if where is not None:          # the noisy frame picks a weave that is clean without the noise
                assert not b["deinterlaced"] and a["metrics"][b["match"]] == 0, (phase, k)
            assert k < 5 or a["dropped"] == b["dropped"], (phase, k)


@pytest.mark.parametrize("depth", [8, 10])
def test_hybrid_clip_video_frames_fall_back_to_the_deinterlacer(depth):
    clip, video = hybrid(depth)
    pics, decided = run_model(clip, depth, True, False, True)
    woven, decided_w = run_model(clip, depth, True, False, False)
    n = len(clip)
    for k in video:
        assert decided[k]["deinterlaced"] and not decided_w[k]["deinterlaced"] and decided[k]["metrics"][3 + decided[k]["match"]] > R.COMB_BLOCK
        nb = (clip[max(k - 1, 0)], clip[k], clip[min(k + 1, n - 1)])
        assert not same_planes(pics[k][1], D.deinterlace(*nb, depth, 0, 0)[0])
        assert not same_planes(woven[k][1], R.weave(clip[k], nb[(1, 0, 2)[decided_w[k]["match"]]], depth, 0))
    others = [k for k, d in enumerate(decided) if d["deinterlaced"] and k not in video]
    assert set(others) <= {min(video) - 1, max(video) + 1}          # (a film frame beside the passage may have lost its partner field)


# ------------------------------------------------------------------------------------------------ 2. the kernel programs stepped on the CPU
@pytest.fixture(scope="module")
def emu():
    lib = util.stepped_library()
    lib.emu_fm_metrics.argtypes = [C.c_void_p] * 3 + [C.c_int] * 6 + [C.c_uint, C.POINTER(C.c_ulonglong), C.POINTER(C.c_int)]
    lib.emu_fm_weave.argtypes = [C.POINTER(C.c_void_p)] * 2 + [C.c_int] * 6 + [C.c_void_p] * 3 + [C.POINTER(C.c_int)]
    lib.emu_fm_tile.argtypes = [C.POINTER(C.c_int)] * 3
    lib.emu_fm_plan.argtypes = [C.POINTER(C.c_ulonglong), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_longlong)]
    lib.emu_fm_plan.restype = C.c_longlong
    return lib


def emu_metrics(emu, size, depth, kind, keep, order=0, align=16, seed=1):
    P, Cc, N = frames(size, depth, kind)
    out, stats = (C.c_ulonglong * 8)(), (C.c_int * 4)()
    rc = emu.emu_fm_metrics(P[0].ctypes.data, Cc[0].ctypes.data, N[0].ctypes.data, size[0], size[1], depth, keep, order, align, seed, out, stats)
    assert rc == 0, rc
    assert stats[0] == 0, f"{stats[0]} misaligned accesses"
    assert stats[2] == align
    return list(out)


def emu_weave(emu, size, depth, kind, keep, order=0, align=16):
    P, Cc, N = frames(size, depth, kind)
    want = R.weave(Cc, N, depth, keep)
    out = [np.full(p.shape, 0x77, p.dtype) for p in want]
    stats = (C.c_int * 4)()
    rc = emu.emu_fm_weave(plane_pointers(Cc), plane_pointers(N), size[0], size[1], depth, keep, order, align, *[p.ctypes.data for p in out], stats)
    assert rc == 0, rc
    assert stats[0] == 0 and stats[1] == 0 and (stats[2], stats[3]) == (align, align), list(stats)
    return same_planes(out, want)


def test_sizes_meet_the_tile_edges(emu):
    tw, th, lds = C.c_int(), C.c_int(), C.c_int()
    emu.emu_fm_tile(C.byref(tw), C.byref(th), C.byref(lds))
    assert tw.value % 32 == 0 and th.value % 32 == 0          # no 16x16 or 32x32 block straddles tiles
    assert 136 > tw.value and 136 % tw.value and 72 > 2 * th.value and 72 % th.value          # 136x72: two tiles across, three down, partial ones
    assert 20 < th.value and 264 > 2 * tw.value                                                # 264x20: fewer rows than a tile
    assert 70 < tw.value and 70 % 8 and 70 % 16 and 36 > th.value                              # 70x36: a run that straddles W, partial blocks, a second tile row
    assert 4 * lds.value <= 160 * 1024


@pytest.mark.parametrize("keep", [0, 1])
@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_stepped_kernels_equal_model(emu, size, depth, keep):
    for kind in ("noise", "film"):
        for order in (0, 1, 2):
            assert emu_metrics(emu, size, depth, kind, keep, order, 16, seed=17 * order + depth) == model_metrics(size, depth, kind, keep), (kind, order)
            diff = emu_weave(emu, size, depth, kind, keep, order)
            assert not diff, (kind, order, diff)


@pytest.mark.parametrize("align", [1, 4, 8])
@pytest.mark.parametrize("depth", [8, 10])
def test_stepped_kernels_with_misaligned_planes(emu, depth, align):
    for i, size in enumerate(SIZES):
        for keep in (0, 1):
            assert emu_metrics(emu, size, depth, "noise", keep, i % 3, align, seed=align + i) == model_metrics(size, depth, "noise", keep), (size, keep)
            diff = emu_weave(emu, size, depth, "noise", keep, i % 3, align)
            assert not diff, (size, keep, diff)


def test_stepped_kernels_clamp_values_above_the_declared_depth():
    assert max(int(p.max()) for f in frames(SIZES[0], 10, "noise") for p in f) > 60000          # what every 10-bit noise case above was fed
    assert model_metrics(SIZES[0], 10, "noise", 0) != R.metrics(*[f[0] & 1023 for f in frames(SIZES[0], 10, "noise")], 10, 0)          # clamped, not masked


def test_stepped_kernels_under_address_sanitizer(tmp_path):
    """a stand-alone program (its own main, no python in the process): the stepped kernels over source planes allocated to end with their last sample, every
    size, element type, alignment class and keep.  A read past a plane ends it with the sanitizer's report"""
    exe = tmp_path / "fieldmatch_asan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-w", "-o", str(exe),
                    str(ROOT / "tests" / "emu" / "fieldmatch.cpp"), str(ROOT / "tests" / "fieldmatch_asan_main.cc")], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert p.stdout.strip() == "80 runs"


# ------------------------------------------------------------------------------------------------ 3. the planner
def test_plan_header_equals_the_restatement(emu):
    rng = np.random.default_rng(5)
    for trial in range(300):
        n = int(rng.integers(1, 18))
        small = trial % 3 == 0          # few distinct values: ties in the comb sums and in (DB, DS)
        mets = []
        for _ in range(n):
            s = rng.integers(0, 3 if small else 1 << 40, 3)
            k = rng.integers(78, 83, 3) if small or trial % 2 else rng.integers(0, 257, 3)
            db = rng.integers(0, 2 if small else 1 << 19)
            mets.append([int(v) for v in s] + [int(v) for v in k] + [int(rng.integers(0, 3 if small else 1 << 30)) + int(db), int(db)])
        for decimate in (0, 1):
            for deint in (0, 1):
                flat = (C.c_ulonglong * (8 * n))(*[v for m in mets for v in m])
                match, fb, dropped, pic = (C.c_int * n)(), (C.c_int * n)(), (C.c_int * n)(), (C.c_longlong * n)()
                pictures = emu.emu_fm_plan(flat, n, decimate, deint, match, fb, dropped, pic)
                want = R.plan(mets, decimate, deint)
                assert [(d["match"], int(d["deinterlaced"]), int(d["dropped"]), d["picture"]) for d in want] == list(zip(match, fb, dropped, pic)), (trial, decimate, deint)
                assert pictures == sum(not d["dropped"] for d in want) == (n - n // 5 if decimate else n)
                assert not want[0]["dropped"]


def test_plan_ties_and_the_first_frame():
    z = [0, 0, 0, 0, 0, 0, 0, 0]
    d = R.plan([z] * 5, True, True)
    assert [f["match"] for f in d] == [0] * 5 and [f["dropped"] for f in d] == [False, True, False, False, False]          # c wins ties; the first frame is never the duplicate
    assert R.plan([[5, 5, 4, 0, 0, 0, 0, 0]], False, True)[0]["match"] == 2 and R.plan([[5, 4, 4, 0, 0, 0, 0, 0]], False, True)[0]["match"] == 1
    assert [f["picture"] for f in R.plan([z] * 9, True, True)] == [0, -1, 1, 2, 3, 4, 5, 6, 7]          # a partial last cycle drops nothing
    assert R.plan([[0, 0, 0, 80, 0, 0, 0, 0]], False, True)[0]["deinterlaced"] is False and R.plan([[0, 0, 0, 81, 0, 0, 0, 0]], False, True)[0]["deinterlaced"] is True
    assert R.plan([[0, 0, 0, 81, 0, 0, 0, 0]], False, False)[0]["deinterlaced"] is False
    lex = [z, [0] * 6 + [9, 2], [0] * 6 + [50, 1], [0] * 6 + [40, 1], [0] * 6 + [40, 1]]
    assert [f["dropped"] for f in R.plan(lex, True, True)] == [False, False, False, True, False]          # DB first, then DS, then the lowest index


# ------------------------------------------------------------------------------------------------ 4. the entry points without a device
def metrics_call(w=64, h=48, depth=8, keep=0, **over):
    fr = D.noise_frames(w, h, depth, 1)
    out = (C.c_uint64 * 8)()
    a = dict(prev=fr[0][0].ctypes.data, cur=fr[1][0].ctypes.data, next=fr[2][0].ctypes.data, w=w, h=h, pitch=w, depth=depth, keep=keep, out=out)
    a.update(over)
    rc = _lib.load().mihevc_k_fieldmatch_metrics(0, a["prev"], a["cur"], a["next"], a["w"], a["h"], a["pitch"], a["depth"], a["keep"], a["out"])
    del fr
    return rc


def weave_call(w=64, h=48, depth=8, keep=0, **over):
    fr = D.noise_frames(w, h, depth, 1)
    pw, ph = R.coded(w), R.coded(h)
    out = [np.zeros(s, R.dtype(depth)) for s in ((ph, pw), (ph // 2, pw // 2), (ph // 2, pw // 2))]
    a = dict(cur=plane_pointers(fr[1]), other=plane_pointers(fr[0]), w=w, h=h, pitch_y=w, pitch_c=w // 2, depth=depth, keep=keep,
             oy=out[0].ctypes.data, ou=out[1].ctypes.data, ov=out[2].ctypes.data)
    a.update(over)
    rc = _lib.load().mihevc_k_fieldmatch_weave(0, a["cur"], a["other"], a["w"], a["h"], a["pitch_y"], a["pitch_c"], a["depth"], a["keep"], a["oy"], a["ou"], a["ov"])
    del fr, out
    return rc


def test_stage_entries_reject_bad_arguments():
    for call, pitches in ((metrics_call, dict(pitch=64)), (weave_call, dict(pitch_y=64, pitch_c=32))):
        for w, h in ((63, 48), (64, 46), (64, 50), (14, 48), (64, 12)):      # odd width, heights that are no multiple of 4, too small
            assert call(w=w, h=h, **pitches) == _lib.EINVAL, (w, h)
        for depth in (9, 12, 16, 0):
            assert call(depth=depth) == _lib.EINVAL
        assert call(keep=2) == _lib.EINVAL and call(keep=-1) == _lib.EINVAL
    assert metrics_call(pitch=63) == _lib.EINVAL and weave_call(pitch_y=63) == _lib.EINVAL and weave_call(pitch_c=31) == _lib.EINVAL
    for k in ("prev", "cur", "next", "out"):
        assert metrics_call(**{k: None}) == _lib.EINVAL, k
    for k in ("cur", "other", "oy", "ou", "ov"):
        assert weave_call(**{k: None}) == _lib.EINVAL, k
    y = np.zeros((48, 64), np.uint8)
    for k in ("cur", "other"):
        assert weave_call(**{k: (C.c_void_p * 3)(y.ctypes.data, None, y.ctypes.data)}) == _lib.EINVAL, k


def test_session_entries_reject_null():
    lib = _lib.load()
    y = np.zeros((48, 64), np.uint8)
    assert lib.mihevc_send_frame_fieldmatch(None, C.byref(_lib.Fieldmatch(1, 1, 1)), y.ctypes.data, y.ctypes.data, y.ctypes.data, 64, 32, 0, 0) == _lib.EINVAL
    assert lib.mihevc_get_fieldmatch_info(None, 0, C.byref(_lib.FmFrame())) == _lib.EINVAL


@pytest.mark.skipif(_lib.load().mihevc_device_count() > 0, reason="a GPU is present")
def test_no_gpu_means_loud_failure():
    assert metrics_call() == _lib.ENODEV and metrics_call(depth=10, keep=1) == _lib.ENODEV
    assert weave_call() == _lib.ENODEV and weave_call(depth=10, keep=1) == _lib.ENODEV
    assert metrics_call(keep=2) == _lib.EINVAL and weave_call(keep=2) == _lib.EINVAL          # the arguments are judged first


def test_layouts_match_the_header(tmp_path):
    src = tmp_path / "sz.c"
    fm = ["sizeof(mihevc_fieldmatch)"] + [f"offsetof(mihevc_fieldmatch,{n})" for n in ("tff", "decimate", "deint", "reserved")]
    names = ("comb_sum", "comb_block", "dup_sum", "dup_block", "match", "deinterlaced", "dropped", "picture")
    fr = ["sizeof(mihevc_fm_frame)"] + [f"offsetof(mihevc_fm_frame,{n})" for n in names]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mihevc.h"\nint main(void){printf("' + "%zu " * (len(fm) + len(fr)) + '\\n",' + ",".join(fm + fr) +
                   ");return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    F, M = _lib.Fieldmatch, _lib.FmFrame
    assert got[:5] == [C.sizeof(F), F.tff.offset, F.decimate.offset, F.deint.offset, F.reserved.offset] and got[0] == 32
    assert got[5:] == [C.sizeof(M)] + [getattr(M, n).offset for n in names]
    assert _lib.load().mihevc_abi_version() == 6
    assert {"mihevc_send_frame_fieldmatch", "mihevc_get_fieldmatch_info", "mihevc_k_fieldmatch_metrics", "mihevc_k_fieldmatch_weave"} <= set(_lib.EXPORTS)


# ------------------------------------------------------------------------------------------------ 5. encode_file(deinterlace='ivtc' | 'match')
from tests.ingest_common import fake_ffmpeg, info          # noqa: E402,F401
from tests.test_deint_cpu import StubEncoder as DeintStub, fake_ffprobe          # noqa: E402,F401


class StubEncoder(DeintStub):
    """stands where the session would: keeps what encode_file hands it, and hands out four pictures for five frames when it decimates"""

    def send_fieldmatch(self, y, u, v, tff=True, decimate=True, deint=True, asynchronous=False, pts=None):
        self.calls.append(("fieldmatch", y.shape, u.shape, str(y.dtype), tff, decimate, deint, pts))
        self.frames = getattr(self, "frames", 0) + 1
        self.sent = self.frames - self.frames // 5 if decimate else self.frames


def test_encode_file_inverse_telecine_in_front_of_the_pipe(fake_ffprobe, fake_ffmpeg, tmp_path, monkeypatch):
    from hevc_amd import encoder, mp4
    w, h, n = 64, 48, 10
    monkeypatch.setenv("FAKE_FRAMES", str(n))
    monkeypatch.setenv("FAKE_FB", str(w * h * 3 // 2))
    monkeypatch.setattr(encoder, "Encoder", StubEncoder)
    seen = []

    def run(out, fps=30000 / 1001, **kw):
        DeintStub.made.clear()
        seen.clear()
        nfo = info("yuv420p", w, h, n)
        nfo.fps = fps
        rc = encoder.encode_file(tmp_path / "a.mov", tmp_path / out, nfo, total_frames=n, progress_callback=lambda name, done, total: seen.append((done, total)), **kw)
        return rc, (DeintStub.made[0] if DeintStub.made else None)

    def samples(path):
        data = path.read_bytes()
        start, end = 0, len(data)
        for name in ("moov", "trak", "mdia", "minf", "stbl", "stsz"):
            _, start, end = [b for b in mp4.parse_boxes(data, start, end) if b[0] == name][0]
        return int.from_bytes(data[start + 8:start + 12], "big")

    # 'ivtc': one call per frame, decimating; the session, its level and the track at exactly 4/5 of the rate; the progress total scaled
    monkeypatch.setenv("FAKE_FIELD_ORDER", "tt")
    rc, enc = run("f.mp4", deinterlace="ivtc")
    argv = fake_ffmpeg.read_text().split("\n")[-2].split()
    assert rc == 0 and not {"-vf", "-filter:v"} & set(argv) and not any("fieldmatch" in a or "decimate" in a for a in argv)
    assert enc.calls == [("fieldmatch", (h, w), (h // 2, w // 2), "uint8", True, True, True, i) for i in range(n)]
    assert (enc.cfg.fps_num, enc.cfg.fps_den) == (24000, 1001)
    assert seen[-1] == (8, 8) and samples(tmp_path / "f.mp4") == 8
    from hevc_amd.transcoder import calculate_apple_hevc_level
    slow = info("yuv420p", w, h, 8)
    slow.fps = 24000 / 1001
    assert enc.cfg.level_idc == int(round(float(calculate_apple_hevc_level(slow)[0]) * 30))
    rc, enc = run("g.mp4", fps=30.0, deinterlace="ivtc")
    assert rc == 0 and (enc.cfg.fps_num, enc.cfg.fps_den) == (24, 1)
    # 'match': the rate stays; bottom field first from the probe; tff= outranks it
    monkeypatch.setenv("FAKE_FIELD_ORDER", "bb")
    rc, enc = run("h.mp4", deinterlace="match")
    assert rc == 0 and enc.calls == [("fieldmatch", (h, w), (h // 2, w // 2), "uint8", False, False, True, i) for i in range(n)]
    assert (enc.cfg.fps_num, enc.cfg.fps_den) == (30000, 1001) and seen[-1] == (n, n) and samples(tmp_path / "h.mp4") == n
    rc, enc = run("i.mp4", deinterlace="match", tff=True)
    assert rc == 0 and all(c[4] is True for c in enc.calls)
    # a source that names no order: top field first
    monkeypatch.setenv("FAKE_FIELD_ORDER", "progressive")
    rc, enc = run("j.mp4", deinterlace="ivtc")
    assert rc == 0 and [c[0] for c in enc.calls] == ["fieldmatch"] * n and all(c[4] is True for c in enc.calls)
    # 'auto' keeps meaning the deinterlacer
    monkeypatch.setenv("FAKE_FIELD_ORDER", "tt")
    rc, enc = run("k.mp4", deinterlace="auto")
    assert rc == 0 and [c[0] for c in enc.calls] == ["deint"] * n
    # refused: size=, native_rgb, denoise=, a height that is no multiple of 4
    for kw in (dict(size=(32, 24)), dict(native_rgb=True), dict(denoise=2)):
        rc, enc = run("m.mp4", **{"deinterlace": "ivtc", **kw})
        assert rc == 1 and (enc is None or not enc.calls), kw
    DeintStub.made.clear()
    monkeypatch.setenv("FAKE_FB", str(w * 46 * 3 // 2))
    assert encoder.encode_file(tmp_path / "a.mov", tmp_path / "n.mp4", info("yuv420p", w, 46, n), total_frames=n, deinterlace="match") == 1
