"""CPU (-m "not gpu"): which options of encode_file go together.  tests/golden/encode_file_combinations.json holds, for every pair of source options, every
dependent option without its owner and chain= beside each of them, what encode_file did in front of a stand-in session, ffmpeg and ffprobe: the return code,
whether a session was made, what it was opened with and which sender took the frames.  The file is a recording of the function as it was before the options
were planned from one table (observe() below made it, run over the old code); this test replays it."""
import ctypes as C
import itertools
import json
from pathlib import Path

import pytest

from hevc_amd import _lib
from tests.ingest_common import info

GOLDEN = Path(__file__).resolve().parent / "golden" / "encode_file_combinations.json"
W, H, N = 64, 48, 3

# a stand-in ffmpeg that answers with frames of the pixel format it is asked for
FFMPEG = f"""#!/bin/sh
case "$*" in *"-pix_fmt gbrp"*) fb={W * H * 3};; *"-pix_fmt yuv422p"*) fb={W * H * 2};; *) fb={W * H * 3 // 2};; esac
case "$*" in
  *"-f rawvideo"*" -") i=0; while [ $i -lt {N} ]; do head -c $fb /dev/zero; i=$((i+1)); done; exit 0;;
esac
for a in "$@"; do last="$a"; done
: > "$last"
"""
FFPROBE = '#!/bin/sh\nprintf \'{"streams":[{"codec_type":"video","field_order":"tt"}]}\'\n'


class Session:
    """stands where Encoder would: one packet per frame, and the name of the sender that took the frames"""
    made = []
    kind = "Encoder"

    def __init__(self, cfg, *a, **kw):
        self.cfg, self.sender, self.sent, self.out = cfg, None, 0, 0
        Session.made.append(self)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass

    def __getattr__(self, name):
        if name.startswith("set_"):
            return lambda *a, **kw: None
        if not name.startswith("send"):
            raise AttributeError(name)

        def send(*a, **kw):
            self.sender, self.sent = name, self.sent + 1
        return send

    def packets_dts(self):
        while self.out < self.sent:
            self.out += 1
            yield b"\x00\x00\x00\x01\x26\x01" + bytes(8), self.out - 1, self.out == 1, self.out - 1

    def flush(self):
        pass

    def headers(self):
        buf = (C.c_uint8 * 4096)()
        n = _lib.load().mihevc_write_parameter_sets(C.byref(self.cfg), buf, 4096)
        assert n > 0
        return bytes(buf[:n])


class Several(Session):
    """stands where ShardedEncoder and SlicedEncoder would"""

    def ready(self):
        return [p[:3] for p in self.packets_dts()]

    finish = ready

    def close(self):
        pass


class Sharded(Several):
    kind = "ShardedEncoder"


class Sliced(Several):
    kind = "SlicedEncoder"


OPTIONS = {"size": dict(size=[32, 24]), "deinterlace": dict(deinterlace="frame"), "denoise": dict(denoise=2), "lut": dict(lut="hdr-to-sdr"),
           "interpolate": dict(interpolate=2), "upscale": dict(upscale=[128, 96]), "sr_model": dict(sr_model="MODEL"), "native_rgb": dict(native_rgb=True),
           "devices": dict(devices=[0, 1]), "row_split": dict(devices=[0, 1], row_split=True)}
VARIANTS = [dict(deinterlace=m) for m in ("field", "auto", "ivtc", "match", "bob")] + [
    dict(denoise=0), dict(denoise=[1, 2, 3, 4]), dict(denoise=4), dict(denoise=0, deinterlace="frame"), dict(lut="hdr-to-sdr", lut_bit_depth=10),
    dict(lut="hdr-to-sdr", lut_bit_depth=12), dict(lut_bit_depth=12), dict(interpolate=5), dict(interpolate=3, interp_mode="blend"),
    dict(interpolate=2, interp_mode="flow"), dict(interp_mode="flow"), dict(upscale="auto"), dict(upscale=96), dict(upscale=[32, 24]), dict(size=[128, 96]),
    dict(row_split=True), dict(devices=[0]), dict(devices=[0], row_split=True), dict(devices=[0], denoise=2), dict(size=[32, 24], upscale=None)]
DEPENDENTS = [dict(tff=True), dict(tff=False, deinterlace="frame"), dict(sr_target="auto"), dict(sr_target=[128, 96]), dict(sr_target=[128, 96], sr_model="MODEL"),
              dict(sr_target=[30, 22], sr_model="MODEL"), dict(sr_denoise=0.5), dict(sr_denoise=0.5, sr_model="MODEL"), dict(sr_model="none.pth"),
              dict(sharpen=65), dict(sharpen=65, upscale=[128, 96]), dict(sharpen=True, upscale=[128, 96]), dict(sharpen=0, upscale=[128, 96]),
              dict(antiring=9), dict(antiring=9, upscale=[128, 96]), dict(antiring=-1, upscale=[128, 96]), dict(antiring=0, upscale=[128, 96])]
CHAIN = dict(denoise=2, interpolate=2)
BESIDE_CHAIN = list(OPTIONS.values()) + [dict(), dict(tff=True), dict(sr_target="auto"), dict(sr_denoise=0.5), dict(sharpen=65), dict(antiring=9), dict(interp_mode="flow"),
                                        dict(lut_bit_depth=12), dict(row_split=True), dict(devices=[0]), dict(denoise=0)]


def cases():
    """(pixel format of the source, options): every case the recording holds, in its order"""
    out = []
    for pix in ("yuv420p", "gbrp"):
        out.append((pix, {}))
        out += [(pix, dict(o)) for o in OPTIONS.values()]
        out += [(pix, {**OPTIONS[a], **OPTIONS[b]}) for a, b in itertools.combinations(OPTIONS, 2)]
        out += [(pix, {**o, "chain": CHAIN}) for o in BESIDE_CHAIN]
    out += [("yuv420p", dict(o)) for o in VARIANTS + DEPENDENTS]
    out += [("yuv420p", {"chain": c}) for c in (dict(), dict(lut="hdr-to-sdr"), dict(deinterlace="ivtc", denoise=2, upscale=[128, 96], interpolate=2),
                                               dict(deinterlace="field", size=[32, 24]), dict(sr_model="MODEL", sr_target=[128, 96]), dict(size=[32, 24], upscale=[128, 96]))]
    out += [("yuv422p", dict(o)) for o in ({}, OPTIONS["size"], OPTIONS["denoise"], OPTIONS["lut"], OPTIONS["sr_model"], OPTIONS["row_split"], {"chain": CHAIN})]
    return out


def set_the_stage(tmp_path, monkeypatch):
    """the stand-ins in place -> (encode_file, a scale 2 model, the directory)"""
    from hevc_amd import encoder, sr
    from tests.test_sr_loader import state_dict
    b = tmp_path / "bin"
    b.mkdir()
    for name, text in (("ffmpeg", FFMPEG), ("ffprobe", FFPROBE)):
        (b / name).write_text(text)
        (b / name).chmod(0o755)
    monkeypatch.setenv("PATH", f"{b}:/usr/bin:/bin")
    monkeypatch.setattr(encoder, "Encoder", Session)
    monkeypatch.setattr(encoder, "ShardedEncoder", Sharded)
    monkeypatch.setattr(encoder, "SlicedEncoder", Sliced)
    return encoder.encode_file, sr.load_rrdbnet(state_dict(2, 1)), tmp_path


@pytest.fixture
def stand_ins(tmp_path, monkeypatch):
    return set_the_stage(tmp_path, monkeypatch)


def observe(stand_ins, pix, options):
    """what encode_file does with these options: the record the golden file keeps"""
    encode_file, model, tmp = stand_ins
    tuples = lambda v: tuple(v) if isinstance(v, list) else v
    kw = {k: tuples(v) for k, v in options.items() if k not in ("devices", "chain")}
    for k in ("devices", "chain"):
        if k in options:
            kw[k] = {n: tuples(v) for n, v in options[k].items()} if isinstance(options[k], dict) else options[k]
    for d in (kw, kw.get("chain") or {}):
        if d.get("sr_model") == "MODEL":
            d["sr_model"] = model
        elif "sr_model" in d:
            d["sr_model"] = tmp / d["sr_model"]
    Session.made.clear()
    try:
        rc = encode_file(tmp / "a.mov", tmp / "o.mp4", info(pix, W, H, N), total_frames=N, **kw)
    except Exception as e:
        rc = type(e).__name__
    enc = Session.made[0] if Session.made else None
    return {"pix": pix, "options": options, "rc": rc, "session": enc is not None and enc.kind, "sender": enc and enc.sender,
            "cfg": enc and [enc.cfg.width, enc.cfg.height, enc.cfg.bit_depth, enc.cfg.fps_num, enc.cfg.fps_den, enc.cfg.matrix, enc.cfg.level_idc], "pictures": enc and enc.out}


def test_the_recording_holds_every_case():
    held = [[r["pix"], r["options"]] for r in json.loads(GOLDEN.read_text())]
    assert held == json.loads(json.dumps(cases())) and len(held) > 200


def test_encode_file_takes_and_refuses_what_it_did(stand_ins):
    for want in json.loads(GOLDEN.read_text()):
        assert observe(stand_ins, want["pix"], want["options"]) == want
