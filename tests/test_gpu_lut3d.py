"""GPU (-m gpu): the colour table source on an MI355X.  The kernel alone (mihevc_k_lut3d) against the numpy model of tests/lut3d_ref.py, bit for bit,
over the sizes, depths, table sizes and inputs of the CPU tests, misaligned planes and one 1080p picture under a 65-point table; sessions fed 10-bit frames
through mihevc_send_frame_lut3d (host planes, asynchronous, device planes, the table replaced in the middle of the clip, mixed with plain frames) give byte for
byte the stream of a session fed the model's pictures through mihevc_send_frame; errors leave the session usable; encode_file(lut='hdr-to-sdr') on a PQ y4m."""
import ctypes as C
import functools
import hashlib
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import lut3d_ref as R
from tests.ingest_common import alignment_class, same_planes, view_of_class
from tests.lut3d_common import CASES, H, N_FRAMES, SIZES, SRC_B, SRC_MATRIX, W, cfg_of, clip, model, model_pictures, session_table, source, src_struct, table, vp

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def lib():
    from hevc_amd import _lib
    L = _lib.load()
    assert L.mihevc_device_count() >= 1, "no gfx950 device visible: the GPU tests need an MI355X"
    return L


# ------------------------------------------------------------------------------------------------ 1. the kernel alone
def k_lut3d(lib, planes, B, matrix, full, tab, D, out_matrix, out_full, pitch=None, wide=0):
    """wide: extra samples per output row, which must come back untouched"""
    h, w = planes[0].shape
    pw, ph = R.coded(w), R.coded(h)
    out = [np.full((s[0], s[1] + wide), 0x77, R.dtype(D)) for s in ((ph, pw), (ph // 2, pw // 2), (ph // 2, pw // 2))]
    pitch = pitch or (w, w // 2)
    rc = lib.mihevc_k_lut3d(0, C.byref(src_struct(B, matrix, full)), tab.shape[0], vp(tab), *[vp(p) for p in planes], pitch[0], pitch[1], w, h, D, out_matrix, out_full,
                            (C.c_void_p * 3)(*[p.ctypes.data for p in out]), (C.c_int * 3)(*[p.shape[1] for p in out]))
    assert rc == 0, rc
    if wide:
        assert all(np.all(p[:, -wide:] == 0x77) for p in out), "samples written past the coded width"
        out = [np.ascontiguousarray(p[:, :-wide]) for p in out]
    return out


@pytest.mark.parametrize("D", [8, 10])
@pytest.mark.parametrize("B", [8, 10, 12])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_stage_equals_model(lib, size, B, D):
    cases = [c for c in CASES if (c.size, c.B, c.D) == (size, B, D)]
    assert len(cases) == 3
    for k, c in enumerate(cases):
        got = k_lut3d(lib, source(c.size, c.B, c.kind, c.n), c.B, c.matrix, c.full, table(c.n), c.D, c.out_matrix, c.out_full, wide=16 * (k % 2))
        diff = same_planes(got, model(c))
        assert not diff, (c, diff)


@pytest.mark.parametrize("cls", [1, 4, 8])
@pytest.mark.parametrize("B", [8, 10])
def test_stage_with_misaligned_planes(lib, B, cls):
    """the planes' addresses and pitches allow chunks of `cls` bytes and no wider"""
    for c in [c for c in CASES if c.B == B and c.kind == "noise" and c.size in (SIZES[1], SIZES[2])][:2]:
        views = [view_of_class(p, cls) for p in source(c.size, c.B, c.kind, c.n)]
        assert all(alignment_class(v.ctypes.data) == alignment_class(v.strides[0]) == cls for v in views) and views[1].strides == views[2].strides
        pitches = (views[0].strides[0] // views[0].itemsize, views[1].strides[0] // views[1].itemsize)
        diff = same_planes(k_lut3d(lib, views, c.B, c.matrix, c.full, table(c.n), c.D, c.out_matrix, c.out_full, pitches), model(c))
        assert not diff, (c, diff)


def test_stage_equals_model_at_1080p_under_65_points(lib):
    """tile counts and index ranges of a real picture, and the table that leaves L1: 1920x1080, 10 bit BT.2020 to 8 bit BT.709, a random 65-point table"""
    src = R.source("noise", 1920, 1080, 10, seed=9)
    diff = same_planes(k_lut3d(lib, src, 10, 9, 0, table(65), 8, 1, 0), R.convert(src, 10, 9, 0, table(65), 8, 1, 0))
    assert not diff, diff


# ------------------------------------------------------------------------------------------------ 2. sessions
ONE, REPLACED, MIXED = (0,) * N_FRAMES, (0, 0, 0, 0, 1, 1, 1), (0, None, 0, 0, None, None, 1)


def drain(enc):
    enc.flush()
    got = list(enc.packets())
    return b"".join(d for d, _, _ in got), [p for _, p, _ in got]


@functools.lru_cache(maxsize=None)
def reference_stream(depth, plan):
    """(stream, pts list) of a session fed the MODEL's pictures, display size, through mihevc_send_frame"""
    from hevc_amd.encoder import Encoder
    with Encoder(cfg_of(depth), device=0) as enc:
        for y, u, v in model_pictures(depth, plan):
            enc.send(y, u, v)
        return drain(enc)


def lut_session(depth, plan, asynchronous):
    from hevc_amd.encoder import Encoder
    current = None
    with Encoder(cfg_of(depth), device=0) as enc:
        assert enc.coded_size() == (104, 72)
        for i, (src, which) in enumerate(zip(clip(), plan)):
            if which is None:
                enc.send(*model_pictures(depth, plan)[i])
                continue
            if which != current:
                enc.set_lut3d(session_table(which))          # no sync in front: the frames already sent are still on their way
                current = which
            enc.send_lut3d(*src, bit_depth=SRC_B, matrix=SRC_MATRIX, asynchronous=asynchronous)
        return drain(enc)


@pytest.mark.parametrize("route", ["sync", "async"])
@pytest.mark.parametrize("depth", [8, 10])
def test_session_stream_equals_the_model_fed_session(lib, depth, route):
    want, want_pts = reference_stream(depth, ONE)
    got, pts = lut_session(depth, ONE, route == "async")
    assert len(want) > 200 and got == want and pts == want_pts and sorted(pts) == list(range(N_FRAMES))


@pytest.mark.parametrize("depth", [8, 10])
def test_table_replaced_in_the_middle_of_the_clip(lib, depth):
    """four frames under a 33-point table, then, without a sync, a 17-point table and three more frames, all asynchronous: a table overwritten under frames in
    flight would change the first four pictures"""
    want, want_pts = reference_stream(depth, REPLACED)
    got, pts = lut_session(depth, REPLACED, True)
    assert len(want) > 200 and got == want and pts == want_pts
    assert want != reference_stream(depth, ONE)[0]


@pytest.mark.parametrize("depth", [8, 10])
def test_mixed_with_plain_frames(lib, depth):
    want, want_pts = reference_stream(depth, MIXED)
    got, pts = lut_session(depth, MIXED, False)
    assert len(want) > 200 and got == want and pts == want_pts


@pytest.fixture(scope="module")
def device_streams():
    """SHA-256 and pts of the streams of sessions fed from torch tensors, from ONE child process in which torch is initialised before the library
    (tests/lut3d_device_child.py says why)"""
    p = subprocess.run([sys.executable, "-s", "-m", "tests.lut3d_device_child"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    return json.loads(p.stdout[p.stdout.index("{"):])


@pytest.mark.parametrize("name,plan", [("one", ONE), ("replaced", REPLACED)])
@pytest.mark.parametrize("depth", [8, 10])
def test_session_fed_device_planes_equals_the_model_fed_session(lib, device_streams, depth, name, plan):
    want, want_pts = reference_stream(depth, plan)
    assert len(want) > 200 and device_streams[f"{depth}-{name}"] == [hashlib.sha256(want).hexdigest(), want_pts]


# ------------------------------------------------------------------------------------------------ 3. errors
def test_bad_calls_leave_the_session_usable(lib):
    from hevc_amd import _lib
    from hevc_amd.encoder import Encoder
    depth = 8
    good = _lib.Lut3dSrc(SRC_B, SRC_MATRIX, 0)
    tab = session_table(0)

    def send(enc, src, planes, pitch_y=W, pitch_c=W // 2, flags=0):
        return lib.mihevc_send_frame_lut3d(enc._s, None if src is None else C.byref(src), *planes, pitch_y, pitch_c, 99, flags)

    with Encoder(cfg_of(depth), device=0) as enc:
        p0 = [q.ctypes.data for q in clip()[0]]
        assert send(enc, good, p0) == _lib.EINVAL                                    # no table set
        for n in (1, 66, -1):
            assert lib.mihevc_set_lut3d(enc._s, n, vp(tab)) == _lib.EINVAL
        assert send(enc, good, p0) == _lib.EINVAL                                    # still none
        enc.set_lut3d(tab)
        enc.set_lut3d(None)
        assert send(enc, good, p0) == _lib.EINVAL                                    # dropped again
        enc.set_lut3d(tab)
        for i, src in enumerate(clip()):
            p = [q.ctypes.data for q in src]
            if i in (0, 2):
                assert send(enc, None, p) == _lib.EINVAL
                for B in (9, 14, 16, 0):
                    assert send(enc, _lib.Lut3dSrc(B, SRC_MATRIX, 0), p) == _lib.EINVAL
                for m in (0, 2, 4, 10):
                    assert send(enc, _lib.Lut3dSrc(SRC_B, m, 0), p) == _lib.EINVAL
                assert send(enc, _lib.Lut3dSrc(SRC_B, SRC_MATRIX, 2), p) == _lib.EINVAL
                for k in range(4):
                    bad = _lib.Lut3dSrc(SRC_B, SRC_MATRIX, 0)
                    bad.reserved[k] = 1
                    assert send(enc, bad, p) == _lib.EINVAL
                assert send(enc, good, p, pitch_y=W - 1) == _lib.EINVAL and send(enc, good, p, pitch_c=W // 2 - 1) == _lib.EINVAL
                assert send(enc, good, p, flags=4) == _lib.EINVAL
                for k in range(3):
                    assert send(enc, good, [None if j == k else q for j, q in enumerate(p)]) == _lib.EINVAL
                    assert send(enc, good, [q + 1 if j == k else q for j, q in enumerate(p)]) == _lib.EINVAL          # misaligned to the 16-bit element
            enc.send_lut3d(*src, bit_depth=SRC_B, matrix=SRC_MATRIX)
        stream, pts = drain(enc)
        assert send(enc, good, p0) == _lib.ESTATE          # after flush
    assert (stream, pts) == reference_stream(depth, ONE)


def test_sizes_and_sessions_the_table_does_not_take(lib):
    """an odd display size, a session whose matrix is unspecified, one band of a picture coded as two slices: MIHEVC_EINVAL, and the session codes on"""
    from hevc_amd import _lib
    from hevc_amd.encoder import Encoder
    good = _lib.Lut3dSrc(8, 1, 0)
    tab = session_table(1)

    def refused(cfg, w, h, set_rc=0):
        y, u, v = (np.zeros(s, np.uint8) for s in ((h, w), ((h + 1) // 2, (w + 1) // 2), ((h + 1) // 2, (w + 1) // 2)))
        with Encoder(cfg, device=0) as enc:
            assert lib.mihevc_set_lut3d(enc._s, tab.shape[0], vp(tab)) == set_rc
            assert lib.mihevc_send_frame_lut3d(enc._s, C.byref(good), y.ctypes.data, u.ctypes.data, v.ctypes.data, w, (w + 1) // 2, 0, 0) == _lib.EINVAL
            for k in range(3):
                assert lib.mihevc_send_frame(enc._s, y.ctypes.data, u.ctypes.data, v.ctypes.data, w, (w + 1) // 2, k) == 0
            assert len(drain(enc)[0]) > 50

    cfg = cfg_of(8)
    cfg.matrix = 2
    refused(cfg, W, H)
    cfg = cfg_of(8)
    cfg.height = 64
    cfg.pic_height, cfg.slice_count, cfg.slice_index = 96, 2, 0
    cfg.slice_ctu_rows[0], cfg.slice_ctu_rows[1] = 2, 1
    cfg.rate_share_q16 = 43691
    refused(cfg, W, 64, set_rc=_lib.EINVAL)


# ------------------------------------------------------------------------------------------------ 4. encode_file
def test_encode_file_hdr_to_sdr_on_a_pq_y4m(lib, tmp_path, monkeypatch):
    """a small synthetic PQ clip at 10 bit becomes an 8-bit stream that says 1/1/1, carries neither SEI 137 nor 144, decodes to the session's reconstruction, and
    holds the pictures of the model under lut3d.hdr_to_sdr(65)"""
    from hevc_amd import encoder, lut3d, probe, yuvio
    from oracle import oracle as O
    w, h, n = 96, 80, 5
    ys, xs = np.mgrid[0:h, 0:w]
    frames = []
    for i in range(n):
        y = 64 + (xs * 8 + ys * 3 + 16 * i) % 700          # PQ code values up to about 1000 cd/m2
        u = 512 + (xs[::2, ::2] + 4 * i) % 120 - 60
        v = 512 + (ys[::2, ::2] * 2 + 3 * i) % 120 - 60
        frames.append(tuple(np.ascontiguousarray(p.astype("<u2")) for p in (y, u, v)))
    src = tmp_path / "master_hdr.y4m"
    yuvio.write_y4m(src, frames, w, h, fps=30, bit_depth=10)
    seen, RealEncoder = [], encoder.Encoder

    class Keeping(RealEncoder):
        """the session of encode_file, keeping its reconstructions and what it put out"""
        def __init__(self, cfg, device=0):
            super().__init__(cfg, device=device, keep_recon=True)
            self.stream = b""
            seen.append(self)

        def packets_dts(self):
            for data, pts, key, dts in super().packets_dts():
                self.stream += data
                yield data, pts, key, dts

        def close(self):
            if self._s:
                self.recs = [self.recon(i) for i in range(n)]
            super().close()

    monkeypatch.setattr(encoder, "Encoder", Keeping)
    info = probe.VideoInfo(w, h, 30.0, "bt2020", "smpte2084", "bt2020nc", "yuv420p10le", "", "", 0, True, "eng", n, n / 30.0)
    out = tmp_path / "deliverable.mp4"
    assert encoder.encode_file(src, out, info, total_frames=n, device=0, lut="hdr-to-sdr") == 0
    (enc,) = seen
    assert (enc.cfg.bit_depth, enc.cfg.hdr10, enc.cfg.matrix) == (8, 0, 1)
    dec, sinfo = O.decode(enc.stream)
    assert len(dec) == n and all(d.same(O.Frame(*r)) for d, r in zip(dec, enc.recs))
    assert (sinfo["vui.colour_primaries"], sinfo["vui.transfer"], sinfo["vui.matrix"], sinfo["vui.full_range"]) == (1, 1, 1, 0)
    assert sinfo["sei.137.size"] is None and sinfo["sei.144.size"] is None and sinfo["sps.profile_idc"] == 1
    tab = lut3d.hdr_to_sdr(65, "pq", 1000.0)
    with RealEncoder(type(enc.cfg).from_buffer_copy(bytes(enc.cfg)), device=0) as ref:
        want = b""
        for i, f in enumerate(frames):
            y, u, v = R.convert(f, 10, 9, 0, tab, 8, 1, 0)
            ref.send(y[:h, :w], u[:h // 2, :w // 2], v[:h // 2, :w // 2], pts=i)
            want += b"".join(d for d, _, _ in ref.packets())
        ref.flush()
        want += b"".join(d for d, _, _ in ref.packets())
    assert len(want) > 200 and enc.stream == want
    assert out.stat().st_size > len(want)
