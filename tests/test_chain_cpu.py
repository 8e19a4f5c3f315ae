"""CPU (-m "not gpu"): the source filter chain.  hevc_amd/csrc/chain_plan.h, through mihevc_chain_plan_for, against the Python restatement of
tests/chain_ref.py over every slot combination, and its descriptor check against the predicates of the single entries' kernel headers; the planner alone under AddressSanitizer and UBSan in a stand-alone program; the struct layouts; what the two
entries decide without a device; what encode_file(chain=...) refuses before it opens a session, and what it opens the session with; and, on the numpy models, the
conditions that keep the equalities of test_gpu_chain.py from being vacuous."""
import ctypes as C
import itertools
import subprocess
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

from hevc_amd import _lib
from tests import chain_common as K
from tests import chain_ref as CR
from tests.ingest_common import fake_ffmpeg, info          # noqa: F401
from tests.test_deint_cpu import StubEncoder as DeintStub, fake_ffprobe          # noqa: F401

ROOT = Path(__file__).resolve().parents[1]
FIELDS = [dict(), dict(field="deint", field_rate=False), dict(field="deint", field_rate=True, tff=False), dict(field="fieldmatch", decimate=True),
          dict(field="fieldmatch", decimate=False, fm_deint=False)]
DENOISES = [dict(), dict(denoise=2), dict(denoise=(255, 0, 3, 9))]
RESIZES = [dict(), dict(resize="scale"), dict(resize="upscale", sharpen=0, antiring=3), dict(resize="sr")]
INTERPS = [dict(), dict(interpolate=2), dict(interpolate=3, interp_mode="blend"), dict(interpolate=4, scene_threshold=0)]
COUNTS = (1, 2, 5, 6, 12)


def lib_plan(chain, src, session, sr_scale=0, matrix=1, frames=0):
    c = _lib.chain(*src, **K.lib_kwargs(chain))
    return _lib.chain_plan(c, *session, matrix=matrix, sr_scale=sr_scale, frames=frames)


# ------------------------------------------------------------------------------------------------ 1. the planner
def test_plan_header_equals_the_restatement_over_every_slot_combination():
    sources = [(52, 36, 8), (100, 68, 8), (200, 136, 8), (100, 68, 10), (100, 70, 8), (400, 272, 8), (24, 16, 8), (26, 20, 8), (404, 68, 8), (100, 16, 10)]
    session = (100, 68, 8)
    seen = {"valid": 0, "refused": 0}
    for f, d, r, i in itertools.product(FIELDS, DENOISES, RESIZES, INTERPS):
        chain = {**f, **d, **r, **i}
        for src in sources:
            for sr_scale in ((0, 2, 4) if r.get("resize") == "sr" else (0,)):
                want = CR.plan(chain, src, session, sr_scale)
                got = lib_plan(chain, src, session, sr_scale)
                assert (got is None) == (want is None), (chain, src, sr_scale)
                seen["valid" if want else "refused"] += 1
                if want is None:
                    continue
                assert Fraction(got.rate_num, got.rate_den) == want["rate"] and np.gcd(got.rate_num, got.rate_den) == 1 and got.stages == want["stages"], chain
                sizes = {s: (got.width[k], got.height[k], got.bit_depth[k]) for k, s in enumerate(CR.STAGES) if got.width[k]}
                assert sizes == want["sizes"], (chain, src)
                for n in COUNTS:
                    assert lib_plan(chain, src, session, sr_scale, frames=n).pictures == want["pictures"](n), (chain, n)
    assert seen["valid"] > 300 and seen["refused"] > 300, seen
    # the partial cycle of inverse telecine, and what the interpolator makes of it
    ivtc = dict(field="fieldmatch", decimate=True)
    assert [lib_plan(ivtc, session, session, frames=n).pictures for n in COUNTS] == [1, 2, 4, 5, 10]
    assert [lib_plan({**ivtc, "interpolate": 2}, session, session, frames=n).pictures for n in COUNTS] == [1, 3, 7, 9, 19]
    p = lib_plan({**ivtc, "interpolate": 2}, session, session)
    assert (p.rate_num, p.rate_den, p.stages, p.pictures) == (8, 5, 2, 0)
    p = lib_plan(dict(field="deint", field_rate=True, interpolate=4), session, session)
    assert (p.rate_num, p.rate_den) == (8, 1)


def test_plan_under_address_sanitizer(tmp_path):
    """a stand-alone program (its own main, no python in the process): chain_plan.h over every slot combination with good and bad descriptors, each in a heap
    block of exactly its size"""
    exe = tmp_path / "chain_asan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-w", "-o", str(exe),
                    str(ROOT / "tests" / "chain_asan_main.cc")], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert p.stdout.strip() == "380160 descriptors, 4784 valid"


def test_descriptor_check_equals_the_entries_own_predicates(tmp_path):
    """chain_plan.h restates rules that the entries keep in their kernel headers (deint_geometry_ok, denoise_strength_ok, scale_geometry_ok, upscale_src_ok,
    sr_yuv_src_ok, mcfi_mode_ok ...): a stand-alone program holds chain_check against those predicates themselves, every knob in and out of its range"""
    exe = tmp_path / "chain_rules"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-w", "-o", str(exe),
                    str(ROOT / "tests" / "chain_rules_main.cc")], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert p.stdout.strip() == "6054048 descriptors, 139736 valid"


# ------------------------------------------------------------------------------------------------ 2. the descriptor check, case by case
def refused(c, session=(100, 68, 8), matrix=1, sr_scale=0):
    out = _lib.ChainPlan()
    return _lib.load().mihevc_chain_plan_for(C.byref(c), *session, matrix, sr_scale, 0, C.byref(out)) == _lib.EINVAL


def test_every_bad_descriptor_is_einval():
    lib = _lib.load()
    out = _lib.ChainPlan()
    good = lambda **kw: _lib.chain(100, 68, 8, **{"denoise": 2, **kw})
    assert not refused(good())
    assert lib.mihevc_chain_plan_for(None, 100, 68, 8, 1, 0, 0, C.byref(out)) == _lib.EINVAL
    assert lib.mihevc_chain_plan_for(C.byref(good()), 100, 68, 8, 1, 0, 0, None) == _lib.EINVAL
    assert lib.mihevc_chain_plan_for(C.byref(good()), 100, 68, 8, 1, 0, -1, C.byref(out)) == _lib.EINVAL
    assert refused(_lib.chain(100, 68, 8))                                                   # no slot on
    for k in range(9):
        c = good()
        c.reserved[k] = 1
        assert refused(c), k
    for name, values in (("field", (-1, 3)), ("denoise_on", (-1, 2)), ("resize", (-1, 4)), ("interpolate_on", (-1, 2))):
        for v in values:
            c = good()
            setattr(c, name, v)
            assert refused(c), (name, v)
    for w, h in ((99, 68), (100, 67), (14, 68), (100, 14), (8194, 68)):                        # odd, below 16, above 8192
        assert refused(_lib.chain(w, h, 8, denoise=2, resize="scale"), session=(w & ~1 or 16, h & ~1 or 16, 8)), (w, h)
    assert refused(_lib.chain(100, 68, 12, denoise=2)) and refused(good(), session=(100, 68, 12)) and refused(good(), session=(100, 68, 9))
    assert refused(good(), session=(101, 68, 8)) and refused(good(), session=(100, 14, 8))
    # without a resize stage the source is the session's
    assert refused(good(), session=(104, 68, 8)) and refused(good(), session=(100, 72, 8)) and refused(good(), session=(100, 68, 10))
    # field: a height that is no multiple of 4, the flags, the reserved words of the struct that is on (and only of that one)
    assert refused(_lib.chain(100, 70, 8, field="deint"), session=(100, 70, 8)) and not refused(_lib.chain(100, 70, 8, denoise=1), session=(100, 70, 8))
    for field, sub, names, nres in (("deint", "deint", ("tff", "field_rate"), 6), ("fieldmatch", "fieldmatch", ("tff", "decimate", "deint"), 5)):
        assert not refused(_lib.chain(100, 68, 8, field=field))
        for name in names:
            for v in (-1, 2):
                c = _lib.chain(100, 68, 8, field=field)
                setattr(getattr(c, sub), name, v)
                assert refused(c), (field, name, v)
        for k in range(nres):
            c = _lib.chain(100, 68, 8, field=field)
            getattr(c, sub).reserved[k] = 1
            assert refused(c), (field, k)
    c = good()
    c.deint.tff, c.fieldmatch.reserved[0], c.interpolate.factor, c.upscale.sharpen, c.sr.matrix = 7, 1, 9, 99, 3      # structs of slots that are off are not looked at
    assert not refused(c)
    # denoise
    for name in ("luma_spatial", "luma_temporal", "chroma_spatial", "chroma_temporal"):
        for v in (-1, 256):
            c = good()
            setattr(c.denoise, name, v)
            assert refused(c), (name, v)
    for k in range(4):
        c = good()
        c.denoise.reserved[k] = 1
        assert refused(c)
    # resize: the ratio rules of the entries, the struct's own fields
    assert not refused(_lib.chain(400, 272, 8, resize="scale")) and refused(_lib.chain(402, 272, 8, resize="scale")) and refused(_lib.chain(98, 68, 8, resize="scale"))
    assert not refused(_lib.chain(26, 18, 8, resize="upscale")) and refused(_lib.chain(24, 18, 8, resize="upscale")) and refused(_lib.chain(102, 68, 8, resize="upscale"))
    assert not refused(_lib.chain(100, 68, 10, resize="scale")) and not refused(_lib.chain(100, 68, 10, resize="upscale"))      # a depth conversion alone
    for name, v in (("sharpen", -1), ("sharpen", 65), ("antiring", -1), ("antiring", 9), ("width", 50), ("height", 34), ("bit_depth", 10)):
        c = _lib.chain(52, 36, 8, resize="upscale")
        setattr(c.upscale, name, v)
        assert refused(c), (name, v)
    for k in range(3):
        c = _lib.chain(52, 36, 8, resize="upscale")
        c.upscale.reserved[k] = 1
        assert refused(c)
    sr = lambda **kw: _lib.chain(52, 36, 8, resize="sr", **kw)
    assert not refused(sr(), sr_scale=2) and not refused(sr(), sr_scale=4) and not refused(_lib.chain(50, 34, 8, resize="sr"), sr_scale=2)
    assert refused(sr()) and refused(sr(), sr_scale=3)                                        # no model
    assert refused(_lib.chain(48, 32, 8, resize="sr"), sr_scale=2)                            # 96x64: a session larger than the network's output
    assert refused(_lib.chain(104, 72, 8, resize="sr"), sr_scale=4)                           # 416x288 into 100x68: more than 4 : 1
    assert refused(sr(), sr_scale=2, matrix=2) and refused(sr(sr_matrix=2), sr_scale=2) and refused(sr(sr_matrix=0), sr_scale=2)
    for name, v in (("full_range", 2), ("full_range", -1), ("width", 50), ("height", 34), ("bit_depth", 10)):
        c = sr()
        setattr(c.sr, name, v)
        assert refused(c, sr_scale=2), (name, v)
    for k in range(3):
        c = sr()
        c.sr.reserved[k] = 1
        assert refused(c, sr_scale=2)
    # interpolate
    for name, v in (("factor", 1), ("factor", 5), ("mode", 2), ("mode", -1), ("scene_threshold", -1), ("scene_threshold", 256)):
        c = good(interpolate=2)
        setattr(c.interpolate, name, v)
        assert refused(c), (name, v)
    for k in range(5):
        c = good(interpolate=2)
        c.interpolate.reserved[k] = 1
        assert refused(c)


def test_the_helper_judges_names_and_types():
    for kw in (dict(field="bob"), dict(resize="lanczos"), dict(denoise=4), dict(denoise=(1, 2, 3)), dict(interpolate=5), dict(interpolate=2, interp_mode="flow"),
               dict(interpolate=True)):
        with pytest.raises(ValueError):
            _lib.chain(100, 68, 8, **kw)
    c = _lib.chain(52, 36, 10, field="fieldmatch", decimate=False, denoise=(1, 2, 3, 4), resize="upscale", sharpen=3, antiring=2, interpolate=3, interp_mode="blend")
    assert (c.field, c.denoise_on, c.resize, c.interpolate_on) == (2, 1, 2, 1)
    assert (c.fieldmatch.tff, c.fieldmatch.decimate, c.fieldmatch.deint) == (1, 0, 1) and c.denoise.chroma_temporal == 4
    assert (c.upscale.width, c.upscale.height, c.upscale.bit_depth, c.upscale.sharpen, c.upscale.antiring) == (52, 36, 10, 3, 2)
    assert (c.interpolate.factor, c.interpolate.mode, c.interpolate.scene_threshold) == (3, 1, 10)


# ------------------------------------------------------------------------------------------------ 3. the entries without a device
def test_session_entries_reject_null():
    lib = _lib.load()
    y = np.zeros((68, 100), np.uint8)
    assert lib.mihevc_set_source_chain(None, C.byref(_lib.chain(100, 68, 8, denoise=2))) == _lib.EINVAL
    assert lib.mihevc_send_frame_chain(None, y.ctypes.data, y.ctypes.data, y.ctypes.data, 100, 50, 0, 0) == _lib.EINVAL


@pytest.mark.skipif(_lib.load().mihevc_device_count() > 0, reason="a GPU is present")
def test_no_gpu_means_no_session_and_the_plan_still_answers():
    from hevc_amd.encoder import Encoder
    with pytest.raises(_lib.MihevcError) as e:
        Encoder(K.cfg_of(8))
    assert e.value.code == _lib.ENODEV
    assert lib_plan(K.FULL[2], (52, 36, 8), (100, 68, 8), frames=12).pictures == 19


def test_layouts_match_the_header(tmp_path):
    src = tmp_path / "sz.c"
    names = ("width", "height", "bit_depth", "field", "denoise_on", "resize", "interpolate_on", "reserved", "deint", "fieldmatch", "denoise", "upscale", "sr", "interpolate")
    pnames = ("rate_num", "rate_den", "stages", "reserved", "pictures", "width", "height", "bit_depth")
    exprs = (["sizeof(mihevc_chain)"] + [f"offsetof(mihevc_chain,{n})" for n in names] + ["sizeof(mihevc_chain_plan)"] + [f"offsetof(mihevc_chain_plan,{n})" for n in pnames] +
             ["MIHEVC_CHAIN_FIELD_NONE", "MIHEVC_CHAIN_FIELD_DEINT", "MIHEVC_CHAIN_FIELD_MATCH", "MIHEVC_CHAIN_RESIZE_NONE", "MIHEVC_CHAIN_RESIZE_SCALE",
              "MIHEVC_CHAIN_RESIZE_UPSCALE", "MIHEVC_CHAIN_RESIZE_SR"])
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mihevc.h"\nint main(void){printf("' + "%zu " * len(exprs) + '\\n",' +
                   ",".join(f"(size_t)({e})" for e in exprs) + ");return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    Ch, P = _lib.Chain, _lib.ChainPlan
    n = 1 + len(names)
    assert got[:n] == [C.sizeof(Ch)] + [getattr(Ch, x).offset for x in names] and got[0] == 256
    assert got[n:n + 1 + len(pnames)] == [C.sizeof(P)] + [getattr(P, x).offset for x in pnames]
    assert got[n + 1 + len(pnames):] == [_lib.CHAIN_FIELD[None], _lib.CHAIN_FIELD["deint"], _lib.CHAIN_FIELD["fieldmatch"], _lib.CHAIN_RESIZE[None],
                                         _lib.CHAIN_RESIZE["scale"], _lib.CHAIN_RESIZE["upscale"], _lib.CHAIN_RESIZE["sr"]]
    assert bytes(_lib.Chain()) == bytes(256)
    assert _lib.load().mihevc_abi_version() == 6
    assert {"mihevc_set_source_chain", "mihevc_send_frame_chain", "mihevc_chain_plan_for"} <= set(_lib.EXPORTS)


# ------------------------------------------------------------------------------------------------ 4. the conditions on the models
@pytest.mark.parametrize("name", sorted(K.MULTI))
def test_dropping_any_one_stage_changes_the_pictures(name):
    case = K.MULTI[name]
    on = CR.stages_on(case[2])
    assert len(on) == (4 if name == "full" else 2)
    whole = K.model(case, 8)
    for stage in on:
        less = K.model(case, 8, chain=CR.without(case[2], stage))
        same = len(less) == len(whole) and all(a.shape == b.shape and np.array_equal(a, b) for (_, p), (_, q) in zip(whole, less) for a, b in zip(p, q))
        assert not same, (name, stage)
    assert [pts for pts, _ in whole] == list(range(len(whole)))
    assert len(whole) == CR.plan(case[2], case[1] + (8,), K.session_size(case) + (8,))["pictures"](K.N_FRAMES)


@pytest.mark.parametrize("depth", [8, 10])
def test_the_fieldmatch_clips_drop_a_frame_and_match_a_neighbour(depth):
    for case in (K.ONE_SLOT["ivtc"], K.TWO_SLOT["ivtc-denoise"], K.FULL):
        pics, decided = K.model(case, depth, with_plan=True)
        assert sum(d["dropped"] for d in decided) == 2 and any(d["match"] in (1, 2) for d in decided) and not decided[0]["dropped"], case[0]
        assert all(d["dropped"] is False for d in decided[10:])          # the partial cycle comes out whole
    _, decided = K.model(K.ONE_SLOT["match"], depth, with_plan=True)
    assert not any(d["dropped"] for d in decided) and any(d["match"] in (1, 2) for d in decided)


@pytest.mark.parametrize("name", ["bob-interp2", "upscale-interp3", "full"])
def test_the_interpolation_clips_have_a_moving_pair(name):
    """the motion-compensated pictures are not the blended ones: some pair moves, and stays under the scene threshold"""
    case = K.MULTI[name]
    mc, blend = K.model(case, 8), K.model(case, 8, chain={**case[2], "interp_mode": "blend"})
    assert len(mc) == len(blend) and any(not np.array_equal(a[1][0], b[1][0]) for a, b in zip(mc, blend))


# ------------------------------------------------------------------------------------------------ 5. encode_file(chain=...)
class StubEncoder(DeintStub):
    """stands where the session would: keeps what encode_file hands it and counts pictures as the plan does"""

    def set_sr_model(self, model):
        self.calls.append(("model", model.scale))

    def set_chain(self, width, height, bit_depth=None, chain=None, **kw):
        self.chain = chain
        self.calls.append(("chain", width, height, bit_depth, chain.field, chain.denoise_on, chain.resize, chain.interpolate_on))

    def send_chain(self, y, u, v, pts=None, asynchronous=False):
        self.calls.append(("frame", y.shape, str(y.dtype), pts))
        self.frames = getattr(self, "frames", 0) + 1
        self.sent = max(_lib.chain_plan(self.chain, self.cfg.width, self.cfg.height, self.cfg.bit_depth, 1, 2, self.frames - 1).pictures, 0)      # the last frame waits

    def flush(self):
        self.sent = _lib.chain_plan(self.chain, self.cfg.width, self.cfg.height, self.cfg.bit_depth, 1, 2, self.frames).pictures


def mp4_samples(path):
    from hevc_amd import mp4
    data = path.read_bytes()
    start, end = 0, len(data)
    for name in ("moov", "trak", "mdia", "minf", "stbl", "stsz"):
        _, start, end = [b for b in mp4.parse_boxes(data, start, end) if b[0] == name][0]
    return int.from_bytes(data[start + 8:start + 12], "big")


def test_encode_file_chain_refusals_and_what_the_session_opens_with(fake_ffprobe, fake_ffmpeg, tmp_path, monkeypatch):
    from hevc_amd import encoder
    from hevc_amd.transcoder import calculate_apple_hevc_level
    w, h, n = 64, 48, 12
    monkeypatch.setenv("FAKE_FRAMES", str(n))
    monkeypatch.setenv("FAKE_FB", str(w * h * 3 // 2))
    monkeypatch.setenv("FAKE_FIELD_ORDER", "tt")
    monkeypatch.setattr(encoder, "Encoder", StubEncoder)
    seen = []

    def run(out, pix="yuv420p", fps=30000 / 1001, **kw):
        DeintStub.made.clear()
        seen.clear()
        nfo = info(pix, w, h, n)
        nfo.fps = fps
        rc = encoder.encode_file(tmp_path / "a.mov", tmp_path / out, nfo, total_frames=n, progress_callback=lambda name, done, total: seen.append((done, total)), **kw)
        return rc, (DeintStub.made[0] if DeintStub.made else None)

    # the whole chain: inverse telecine, denoise, enlarge, double the rate.  12 frames: 10 film pictures, 19 out; 30000/1001 x 8/5 = 48000/1001, exactly
    rc, enc = run("a.mp4", chain=dict(deinterlace="ivtc", denoise=2, upscale=(128, 96), sharpen=4, interpolate=2))
    assert rc == 0 and (enc.cfg.width, enc.cfg.height) == (128, 96) and (enc.cfg.fps_num, enc.cfg.fps_den) == (48000, 1001)
    assert enc.calls[0] == ("chain", w, h, 8, 2, 1, 2, 1) and enc.calls[1:] == [("frame", (h, w), "uint8", i) for i in range(n)]
    assert (enc.chain.fieldmatch.tff, enc.chain.fieldmatch.decimate, enc.chain.upscale.sharpen, enc.chain.upscale.antiring, enc.chain.interpolate.factor) == (1, 1, 4, 8, 2)
    assert seen[-1] == (19, 19) and mp4_samples(tmp_path / "a.mp4") == 19
    fast = info("yuv420p", 128, 96, 19)
    fast.fps = 48000 / 1001
    assert enc.cfg.level_idc == int(round(float(calculate_apple_hevc_level(fast)[0]) * 30))
    argv = fake_ffmpeg.read_text().split("\n")[-2].split()
    assert not {"-vf", "-filter:v", "-s"} & set(argv)
    # field rate into a reduction: twice the rate, the probed field order (bottom first), an integer rate stays a float product
    monkeypatch.setenv("FAKE_FIELD_ORDER", "bb")
    rc, enc = run("b.mp4", fps=25.0, chain=dict(deinterlace="field", size=(32, 24)))
    assert rc == 0 and (enc.cfg.width, enc.cfg.height, enc.cfg.fps_num // enc.cfg.fps_den) == (32, 24, 50) and enc.calls[0] == ("chain", w, h, 8, 1, 0, 1, 0)
    assert (enc.chain.deint.tff, enc.chain.deint.field_rate) == (0, 1) and seen[-1] == (24, 24) and mp4_samples(tmp_path / "b.mp4") == 24
    rc, enc = run("c.mp4", chain=dict(deinterlace="frame", tff=True, denoise=(1, 2, 3, 4)))
    assert rc == 0 and enc.chain.deint.tff == 1 and enc.chain.denoise.chroma_temporal == 4 and seen[-1] == (n, n)
    # a 10-bit source
    monkeypatch.setenv("FAKE_FB", str(w * h * 3))
    rc, enc = run("d.mp4", pix="yuv420p10le", chain=dict(denoise=1, interpolate=3, interp_mode="blend"))
    assert rc == 0 and enc.cfg.bit_depth == 10 and enc.calls[0] == ("chain", w, h, 10, 0, 1, 0, 1) and enc.calls[1][2] == "uint16" and seen[-1] == (34, 34)
    monkeypatch.setenv("FAKE_FB", str(w * h * 3 // 2))
    # refused, each before a session exists: chain= beside an option outside the dict, native_rgb, lut=, several devices
    ok = dict(denoise=2, interpolate=2)
    for kw in (dict(size=(32, 24)), dict(deinterlace="frame"), dict(tff=True), dict(denoise=1), dict(interpolate=2), dict(upscale=(128, 96)), dict(sr_model="x.pth"),
               dict(sr_target="auto"), dict(sr_denoise=0.5), dict(native_rgb=True), dict(lut="hdr-to-sdr"), dict(devices=[0, 1]), dict(devices=[0, 1], row_split=True)):
        rc, enc = run("r.mp4", chain=ok, **kw)
        assert rc == 1 and enc is None, kw
    # and what the dict itself may not hold
    for bad in (dict(), dict(denoise=0), dict(lut="x.cube"), dict(denoise=5), dict(denoise=(1, 2, 3)), dict(deinterlace="bob"), dict(tff=True), dict(interpolate=5),
                dict(interpolate=2, interp_mode="flow"), dict(interp_mode="mc"), dict(size=(32, 24), upscale=(128, 96)), dict(size=(30, 24, 1)), dict(size=(8, 8)),
                dict(size=(128, 96)), dict(upscale=(32, 24)), dict(upscale=(300, 96)), dict(upscale="best"), dict(upscale=(128, 96), sharpen=65), dict(sharpen=3),
                dict(upscale=(128, 96), antiring=True), dict(sr_target="auto"), dict(sr_denoise=0.5), dict(sr_model=str(tmp_path / "none.pth")), dict(size=(33, 24)),
                ["denoise"], dict(deinterlace="frame", size=(32, 24), denoise=2, interpolate=2, extra=1)):
        rc, enc = run("s.mp4", chain=bad)
        assert rc == 1 and enc is None, bad
    # a source the chain does not take: 4:2:2, and a height that is no multiple of 4 under a field stage
    monkeypatch.setenv("FAKE_FB", str(w * h * 2))
    rc, enc = run("t.mp4", pix="yuv422p", chain=ok)
    assert rc == 1 and enc is None
    DeintStub.made.clear()
    monkeypatch.setenv("FAKE_FB", str(w * 46 * 3 // 2))
    assert encoder.encode_file(tmp_path / "a.mov", tmp_path / "u.mp4", info("yuv420p", w, 46, n), total_frames=n, chain=dict(deinterlace="match", denoise=1)) == 1
    assert not DeintStub.made
    # the existing options keep refusing each other exactly as before
    rc, enc = run("v.mp4", deinterlace="ivtc", denoise=2)
    assert rc == 1 and enc is None
