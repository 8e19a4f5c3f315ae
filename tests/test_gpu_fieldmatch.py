"""GPU (-m gpu): inverse telecine on an MI355X.  The kernels alone (mihevc_k_fieldmatch_metrics, mihevc_k_fieldmatch_weave) against the numpy
model of tests/fieldmatch_ref.py, bit for bit, over the sizes of the CPU tests, misaligned planes and one 1080p picture; sessions fed telecined frames through
mihevc_send_frame_fieldmatch (synchronous, asynchronous, device planes) give byte for byte the stream of a session fed the model's pictures through
mihevc_send_frame; a clean 10-frame clip gives byte for byte the stream of its 8 film frames; mihevc_get_fieldmatch_info tells the model's decisions; errors
leave the session usable."""
import ctypes as C
import functools
import hashlib
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import deint_ref as D
from tests import fieldmatch_ref as R
from tests.deint_common import plane_pointers
from tests.fieldmatch_common import H, N_FRAMES, SIZES, W, cfg_of, clip, film, frames, hybrid, model_metrics, model_pictures, telecined
from tests.ingest_common import alignment_class, same_planes, view_of_class

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def lib():
    from hevc_amd import _lib
    L = _lib.load()
    assert L.mihevc_device_count() >= 1, "no gfx950 device visible: the GPU tests need an MI355X"
    return L


# ------------------------------------------------------------------------------------------------ 1. the kernels alone
def k_metrics(lib, P, Cc, N, depth, keep, pitch=None):
    h, w = Cc.shape
    out = (C.c_uint64 * 8)()
    rc = lib.mihevc_k_fieldmatch_metrics(0, P.ctypes.data, Cc.ctypes.data, N.ctypes.data, w, h, pitch or w, depth, keep, out)
    assert rc == 0, rc
    return list(out)


def k_weave(lib, cur, other, depth, keep, pitch=None):
    h, w = cur[0].shape
    pw, ph = R.coded(w), R.coded(h)
    out = [np.full(s, 0x77, R.dtype(depth)) for s in ((ph, pw), (ph // 2, pw // 2), (ph // 2, pw // 2))]
    pitch = pitch or (w, w // 2)
    rc = lib.mihevc_k_fieldmatch_weave(0, plane_pointers(cur), plane_pointers(other), w, h, pitch[0], pitch[1], depth, keep, *[p.ctypes.data for p in out])
    assert rc == 0, rc
    return out


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_stages_equal_model(lib, size, depth):
    for kind in ("noise", "film"):
        P, Cc, N = frames(size, depth, kind)
        for keep in (0, 1):
            assert k_metrics(lib, P[0], Cc[0], N[0], depth, keep) == model_metrics(size, depth, kind, keep), (kind, keep)
            diff = same_planes(k_weave(lib, Cc, N, depth, keep), R.weave(Cc, N, depth, keep))
            assert not diff, (kind, keep, diff)


@pytest.mark.parametrize("cls", [1, 4, 8])
@pytest.mark.parametrize("depth", [8, 10])
def test_stages_with_misaligned_planes(lib, depth, cls):
    """the planes' addresses and pitches allow chunks of `cls` bytes and no wider"""
    for size, keep in ((SIZES[0], 0), (SIZES[1], 1)):
        views = [[view_of_class(p, cls) for p in f] for f in frames(size, depth, "noise")]
        assert all(alignment_class(v.ctypes.data) == alignment_class(v.strides[0]) == cls for f in views for v in f)
        pitches = (views[0][0].strides[0] // views[0][0].itemsize, views[0][1].strides[0] // views[0][1].itemsize)
        assert k_metrics(lib, views[0][0], views[1][0], views[2][0], depth, keep, pitches[0]) == model_metrics(size, depth, "noise", keep), size
        P, Cc, N = frames(size, depth, "noise")
        diff = same_planes(k_weave(lib, views[1], views[0], depth, keep, pitches), R.weave(Cc, P, depth, keep))
        assert not diff, (size, diff)


def test_stages_equal_model_at_1080p(lib):
    """tile counts and index ranges of a real picture: 1920x1080, 8 bit (1080 = 33 tile rows and 24 rows more)"""
    P, Cc, N = D.noise_frames(1920, 1080, 8, 7)
    assert k_metrics(lib, P[0], Cc[0], N[0], 8, 1) == R.metrics(P[0], Cc[0], N[0], 8, 1)
    diff = same_planes(k_weave(lib, Cc, P, 8, 1), R.weave(Cc, P, 8, 1))
    assert not diff, diff


# ------------------------------------------------------------------------------------------------ 2. sessions
def drain(enc):
    enc.flush()
    got = list(enc.packets())
    return b"".join(d for d, _, _ in got), [p for _, p, _ in got]


def plain_stream(depth, pictures):
    """(stream, pts list) of a session fed display-size pictures [(pts, planes)] through mihevc_send_frame"""
    from hevc_amd.encoder import Encoder
    with Encoder(cfg_of(depth), device=0) as enc:
        for pts, (y, u, v) in pictures:
            enc.send(np.ascontiguousarray(y), np.ascontiguousarray(u), np.ascontiguousarray(v), pts=pts)
        return drain(enc)


@functools.lru_cache(maxsize=None)
def reference_stream(depth, tff, decimate, deint=True, n=N_FRAMES, which="clip"):
    return plain_stream(depth, model_pictures(depth, tff, decimate, deint, n, which)[0])


def same_info(enc, decided, decimate):
    for k, d in enumerate(decided):
        f = enc.fieldmatch_info(k)
        assert f is not None, k
        got = (list(f.comb_sum) + list(f.comb_block) + [f.dup_sum, f.dup_block], f.match, f.deinterlaced, f.dropped, f.picture)
        assert got == (d["metrics"], d["match"], int(d["deinterlaced"]), int(d["dropped"]), d["picture"]), (k, got, d)


@pytest.mark.parametrize("route", ["sync", "async"])
@pytest.mark.parametrize("decimate", [False, True], ids=["match", "ivtc"])
@pytest.mark.parametrize("tff", [True, False], ids=["tff", "bff"])
@pytest.mark.parametrize("depth", [8, 10])
def test_session_stream_equals_the_model_fed_session(lib, depth, tff, decimate, route):
    from hevc_amd.encoder import Encoder
    want, want_pts = reference_stream(depth, tff, decimate)
    decided = model_pictures(depth, tff, decimate)[1]
    with Encoder(cfg_of(depth), device=0) as enc:
        for i, src in enumerate(clip(depth, tff)):
            enc.send_fieldmatch(*src, tff=tff, decimate=decimate, asynchronous=route == "async")
            assert enc.stats().frames_in == ((i // 5) * 4 if decimate else i)          # pictures; a cycle's four come with its fifth frame's successor
            assert enc.fieldmatch_info(i) is None                                         # undecided until the next frame arrives
        got, pts = drain(enc)
        assert enc.stats().frames_in == len(want_pts) == (N_FRAMES - N_FRAMES // 5 if decimate else N_FRAMES)
        same_info(enc, decided, decimate)
    assert len(want) > 200 and got == want
    assert pts == want_pts == list(range(len(want_pts)))


@pytest.fixture(scope="module")
def device_streams():
    """SHA-256 and pts of the streams of sessions fed from torch tensors, from ONE child process in which torch is initialised before the library
    (tests/fieldmatch_device_child.py says why): what this test is about is that order"""
    p = subprocess.run([sys.executable, "-s", "-m", "tests.fieldmatch_device_child"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    return json.loads(p.stdout[p.stdout.index("{"):])


@pytest.mark.parametrize("decimate", [False, True], ids=["match", "ivtc"])
@pytest.mark.parametrize("tff", [True, False], ids=["tff", "bff"])
@pytest.mark.parametrize("depth", [8, 10])
def test_session_fed_device_planes_equals_the_model_fed_session(lib, device_streams, depth, tff, decimate):
    want, want_pts = reference_stream(depth, tff, decimate)
    assert len(want) > 200 and device_streams[f"{depth}-{int(tff)}-{int(decimate)}"] == [hashlib.sha256(want).hexdigest(), want_pts]


@pytest.mark.parametrize("depth", [8, 10])
def test_recovery_a_clean_clip_codes_exactly_its_film_frames(lib, depth):
    """the 10-frame clip that starts on a clean frame, decimated: byte for byte the stream of a plain session fed its 8 film frames"""
    from hevc_amd.encoder import Encoder
    frames10, src = telecined(depth, 10, 0)
    want, want_pts = plain_stream(depth, list(enumerate(film(depth, 8))))
    with Encoder(cfg_of(depth), device=0) as enc:
        for f in frames10:
            enc.send_fieldmatch(*f, tff=True, decimate=True)
        got, pts = drain(enc)
        assert [enc.fieldmatch_info(k).dropped for k in range(10)] == [0, 0, 1, 0, 0] * 2
        assert [enc.fieldmatch_info(k).deinterlaced for k in range(10)] == [0] * 10
    assert len(want) > 200 and got == want and pts == want_pts == list(range(8))


@pytest.mark.parametrize("deint", [True, False], ids=["deint", "woven"])
def test_hybrid_clip(lib, deint):
    """the video frames in the middle come out as the deinterlacer's pictures, and with deint = 0 as woven"""
    from hevc_amd.encoder import Encoder
    frames12, video = hybrid(8)
    want, want_pts = reference_stream(8, True, False, deint, N_FRAMES, "hybrid")
    decided = model_pictures(8, True, False, deint, N_FRAMES, "hybrid")[1]
    assert all(decided[k]["deinterlaced"] == deint for k in video)
    with Encoder(cfg_of(8), device=0) as enc:
        for f in frames12:
            enc.send_fieldmatch(*f, tff=True, decimate=False, deint=deint)
        got, pts = drain(enc)
        same_info(enc, decided, False)
    assert len(want) > 200 and got == want and pts == want_pts


@pytest.mark.parametrize("n", [1, 4, 5, 6])
def test_short_clips(lib, n):
    """P = C = N for one frame; a partial cycle comes out whole; five frames drop one; the sixth opens a cycle that flush closes"""
    from hevc_amd.encoder import Encoder
    want, want_pts = reference_stream(8, True, True, True, n)
    decided = model_pictures(8, True, True, True, n)[1]
    with Encoder(cfg_of(8), device=0) as enc:
        for f in clip(8, True, n):
            enc.send_fieldmatch(*f, tff=True, decimate=True)
        assert enc.stats().frames_in == (4 if n == 6 else 0)
        got, pts = drain(enc)
        same_info(enc, decided, True)
    assert len(want) > 100 and got == want and pts == want_pts == list(range(n - n // 5))


# ------------------------------------------------------------------------------------------------ 3. errors
def test_bad_calls_leave_the_session_usable(lib):
    from hevc_amd import _lib
    from hevc_amd.encoder import Encoder
    depth, tff = 8, True
    good = _lib.Fieldmatch(1, 1, 1)

    def send(enc, mode, planes, pitch_y=W, pitch_c=W // 2, flags=0):
        return lib.mihevc_send_frame_fieldmatch(enc._s, None if mode is None else C.byref(mode), *planes, pitch_y, pitch_c, 99, flags)

    with Encoder(cfg_of(depth), device=0) as enc:
        assert lib.mihevc_get_fieldmatch_info(enc._s, 0, C.byref(_lib.FmFrame())) == _lib.EINVAL          # never sent
        for i, src in enumerate(clip(depth, tff)):
            p = [q.ctypes.data for q in src]
            if i in (0, 2):          # before the first frame fixes the mode, and with a frame pending
                assert send(enc, None, p) == _lib.EINVAL
                for bad in (_lib.Fieldmatch(2, 1, 1), _lib.Fieldmatch(-1, 1, 1), _lib.Fieldmatch(1, 2, 1), _lib.Fieldmatch(1, 1, -1), _lib.Fieldmatch(1, 1, 2)):
                    assert send(enc, bad, p) == _lib.EINVAL, bad
                for k in range(5):
                    bad = _lib.Fieldmatch(1, 1, 1)
                    bad.reserved[k] = 1
                    assert send(enc, bad, p) == _lib.EINVAL
                assert send(enc, good, p, pitch_y=W - 1) == _lib.EINVAL and send(enc, good, p, pitch_c=W // 2 - 1) == _lib.EINVAL
                assert send(enc, good, p, flags=4) == _lib.EINVAL
                for k in range(3):
                    assert send(enc, good, [None if j == k else q for j, q in enumerate(p)]) == _lib.EINVAL
            if i == 2:               # the mode of the first frame holds; every other entry must wait for flush
                for other in (_lib.Fieldmatch(0, 1, 1), _lib.Fieldmatch(1, 0, 1), _lib.Fieldmatch(1, 1, 0)):
                    assert send(enc, other, p) == _lib.EINVAL
                assert lib.mihevc_get_fieldmatch_info(enc._s, 2, C.byref(_lib.FmFrame())) == _lib.EINVAL
                assert lib.mihevc_get_fieldmatch_info(enc._s, 1, C.byref(_lib.FmFrame())) == _lib.EAGAIN
            if i in (2, 5):          # inside a cycle, and between two cycles with nothing held
                assert lib.mihevc_send_frame(enc._s, *p, W, W // 2, 99) == _lib.ESTATE
                assert lib.mihevc_send_frame_async(enc._s, *p, W, W // 2, 99) == _lib.ESTATE
                assert lib.mihevc_send_frame_device(enc._s, *p, W, W // 2, 99) == _lib.ESTATE
                assert lib.mihevc_send_frame_fmt(enc._s, C.byref(_lib.SrcFormat(422, 0, 8, 0)), *p, W, W // 2, 99, 0) == _lib.ESTATE
                assert lib.mihevc_send_frame_scaled(enc._s, C.byref(_lib.ScaleSrc(W, H, 8)), *p, W, W // 2, 99, 0) == _lib.ESTATE
                assert lib.mihevc_send_frame_deint(enc._s, C.byref(_lib.Deint(1, 0)), *p, W, W // 2, 99, 0) == _lib.ESTATE
                assert lib.mihevc_send_frame_denoise(enc._s, C.byref(_lib.denoise_level(1)), *p, W, W // 2, 99, 0) == _lib.ESTATE
            enc.send_fieldmatch(*src, tff=tff, decimate=True)
        stream, pts = drain(enc)
        assert send(enc, good, [q.ctypes.data for q in clip(depth, tff)[0]]) == _lib.ESTATE
    assert (stream, pts) == reference_stream(depth, tff, True)
    # while a deinterlaced or a denoised frame is pending this entry waits for flush
    p = [q.ctypes.data for q in clip(depth, tff)[0]]
    for first in ("deint", "denoise"):
        with Encoder(cfg_of(depth), device=0) as enc:
            if first == "deint":
                enc.send_deint(*clip(depth, tff)[0], tff=tff)
            else:
                enc.send_denoise(*clip(depth, tff)[0], strength=1)
            assert send(enc, good, p) == _lib.ESTATE
            assert len(drain(enc)[0]) > 50
    # sizes the filter does not take: a height that is no multiple of 4; one band of a picture coded as two slices
    y, u, v = (np.zeros(s, np.uint8) for s in ((70, W), (35, W // 2), (35, W // 2)))
    cfg = cfg_of(depth)
    cfg.height = 70
    with Encoder(cfg, device=0) as enc:
        assert send(enc, good, [y.ctypes.data, u.ctypes.data, v.ctypes.data]) == _lib.EINVAL
        for k in range(3):
            enc.send(y, u, v)
        assert len(drain(enc)[0]) > 50
    cfg = cfg_of(depth)
    cfg.height = 64
    cfg.pic_height, cfg.slice_count, cfg.slice_index = 96, 2, 0
    cfg.slice_ctu_rows[0], cfg.slice_ctu_rows[1] = 2, 1
    cfg.rate_share_q16 = 43691
    with Encoder(cfg, device=0) as enc:
        assert send(enc, good, [y.ctypes.data, u.ctypes.data, v.ctypes.data]) == _lib.EINVAL
        for k in range(3):
            enc.send(y[:64], u[:32], v[:32])
        assert len(drain(enc)[0]) > 50
