"""GPU (-m gpu): how the source entries of a session follow one another.  The per-filter tests cover each entry alone; this one pins what a session answers
when two entries alternate.  For every ordered pair (A, B) of the entries below a 64x64 8-bit session (keyint 4, one lane) is sent a frame through A, one through
B and one more through A, then flushed and drained; the three return codes, the return code of the flush, the number of packets and their pts must equal
tests/golden/source_order.json.  The fixture was recorded once, with the library as it was before the source front end moved into csrc/source.cpp
(`python -m tests.test_gpu_source_order --record`); the packets' content is covered by the per-filter session tests and is not compared here.

Entries: plain host, plain device, _fmt (4:2:2 8 bit), _rgb, _lut3d (a 2-point identity table), _scaled (from 128x128), _upscaled (from 32x32), _deint, _denoise,
_interpolate (factor 2), _fieldmatch (decimate off) and _sr (16x16 through the one-block x4 model of tests/sr_common.py, which packs in a few milliseconds)."""
import ctypes as C
import functools
import json
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
FIXTURE = ROOT / "tests" / "golden" / "source_order.json"
W = H = 64
PTS = (0, 10, 20)      # of the three frames: far enough apart for the second picture of an interpolated or field-rate frame
ENTRIES = ("host", "device", "fmt", "rgb", "lut3d", "scaled", "upscaled", "deint", "denoise", "interpolate", "fieldmatch", "sr")


def picture(w, h, seed):
    """planar 4:2:0, 8 bit: a gradient that moves with `seed`, plus noise"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    y = ((xx * 3 + yy * 2 + 7 * seed) % 200 + rng.integers(0, 40, (h, w))).astype(np.uint8)
    return [np.ascontiguousarray(y), np.ascontiguousarray(y[::2, ::2] // 2 + 60), np.ascontiguousarray(y[1::2, 1::2] // 2 + 70)]


@functools.lru_cache(maxsize=None)
def device_planes():
    """one picture in device memory for the life of the process, put there with the HIP runtime libmihevc itself links (no second runtime in the process): the
    plain device entry codes from the caller's planes where they are, so they must outlive the packets"""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipSetDevice(0) == 0
    out = []
    for pl in picture(W, H, 5):
        d = C.c_void_p()
        assert hip.hipMalloc(C.byref(d), pl.nbytes) == 0
        assert hip.hipMemcpy(d, pl.ctypes.data_as(C.c_void_p), pl.nbytes, 1) == 0      # hipMemcpyHostToDevice
        out.append(d.value)
    return tuple(out)


class Sender:
    """one session and the twelve ways into it; every call returns the entry's return code"""

    def __init__(self):
        from hevc_amd import _lib, lut3d
        from hevc_amd.encoder import Encoder
        from tests import sr_common
        self._lib = _lib
        cfg = _lib.default_config()
        cfg.width, cfg.height, cfg.bit_depth, cfg.keyint, cfg.gops_in_flight = W, H, 8, 4, 1
        self.enc = Encoder(cfg, device=0)
        self.enc.set_lut3d(lut3d.identity(2))
        self.enc.set_sr_model(sr_common.session_model(4))

    def close(self):
        self.enc.close()

    def send(self, entry, pts, seed):
        e, L = self.enc, self._lib
        y, u, v = picture(W, H, seed)
        try:
            if entry == "host":
                e.send(y, u, v, pts=pts)
            elif entry == "device":
                e.send_device(*device_planes(), W, W // 2, pts=pts)
            elif entry == "fmt":
                e.send_fmt(L.SrcFormat(422, 0, 8, 0), y, np.repeat(u, 2, 0), np.repeat(v, 2, 0), pts=pts)
            elif entry == "rgb":
                e.send_rgb(L.rgb_format_for("gbrp"), y, y[::-1].copy(), y[:, ::-1].copy(), pts=pts)
            elif entry == "lut3d":
                e.send_lut3d(y, u, v, 8, 1, pts=pts)
            elif entry == "scaled":
                e.send_scaled(128, 128, *picture(128, 128, seed), pts=pts)
            elif entry == "upscaled":
                e.send_upscaled(32, 32, *picture(32, 32, seed), pts=pts)
            elif entry == "deint":
                e.send_deint(y, u, v, pts=pts)
            elif entry == "denoise":
                e.send_denoise(y, u, v, pts=pts)
            elif entry == "interpolate":
                e.send_interpolate(y, u, v, factor=2, pts=pts)
            elif entry == "fieldmatch":
                e.send_fieldmatch(y, u, v, decimate=False, pts=pts)
            elif entry == "sr":
                s = picture(16, 16, seed)[0]
                e.send_sr(L.rgb_format_for("gbrp"), 16, 16, s, s[::-1].copy(), s[:, ::-1].copy(), pts=pts)
            else:
                raise KeyError(entry)
        except L.MihevcError as err:
            return err.code
        return 0


def run_pair(a, b):
    s = Sender()
    try:
        rcs = [s.send(entry, pts, seed) for seed, (entry, pts) in enumerate(zip((a, b, a), PTS))]
        try:
            s.enc.flush()
            flush = 0
        except s._lib.MihevcError as err:
            flush = err.code
        pts = [p for _, p, _ in s.enc.packets()]
    finally:
        s.close()
    return {"send": rcs, "flush": flush, "packets": len(pts), "pts": pts}


def run_matrix():
    return {f"{a}>{b}": run_pair(a, b) for a in ENTRIES for b in ENTRIES}


@pytest.fixture(scope="module")
def matrix():
    from hevc_amd import _lib
    assert _lib.load().mihevc_device_count() >= 1, "no gfx950 device visible: the GPU tests need an MI355X"
    return run_matrix()


def test_fixture_covers_every_pair():
    want = json.loads(FIXTURE.read_text())
    assert sorted(want) == sorted(f"{a}>{b}" for a in ENTRIES for b in ENTRIES)
    assert all(r["send"][0] == 0 for r in want.values()), "the first frame of a fresh session is accepted by every entry"
    assert any(r["send"][1] != 0 for r in want.values()) and any(r["packets"] > 3 for r in want.values()), "refusals and two-picture frames are in the record"


def test_pairs_answer_as_recorded(matrix):
    want = json.loads(FIXTURE.read_text())
    wrong = {k: (matrix[k], want[k]) for k in want if matrix[k] != want[k]}
    assert not wrong, wrong


if __name__ == "__main__":
    sys.path.insert(0, str(ROOT))
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python -m tests.test_gpu_source_order --record")
    import time
    t0 = time.time()
    got = run_matrix()
    FIXTURE.write_text("{\n" + ",\n".join(' "%s": %s' % (k, json.dumps(got[k], sort_keys=True)) for k in sorted(got)) + "\n}\n")      # one pair per line
    print("recorded %d pairs in %.1f s" % (len(got), time.time() - t0))
