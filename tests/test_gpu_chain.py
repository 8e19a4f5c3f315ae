"""GPU (-m gpu): the source filter chain on an MI355X.  The method is the single filters': the stream and the pts list of a session fed its
source frames through mihevc_send_frame_chain equal, byte for byte, those of a session fed the pictures of the numpy models (tests/chain_ref.py composes them and
nothing else) through mihevc_send_frame.  Every one-slot chain also equals the session of the filter's own entry; the chains with the network equal sessions fed
through mihevc_send_frame_sr_yuv and through the stage entries; synchronous, asynchronous and device planes give one stream; short clips, a flush with every ring
pending, refusals that leave the session coding on, and encode_file(chain=...).

Sizes (tests/chain_common.py): 52x36 into a 100x68 session (coded 104x72) where a chain enlarges, 200x136 into 100x68 where it reduces, 100x68 throughout
otherwise; 12 frames, so two cycles of inverse telecine and a partial one occur.  tests/test_chain_cpu.py checks on the models that no equality here is vacuous."""
import ctypes as C
import functools
import hashlib
import json
import subprocess
import sys
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

from tests import chain_common as K
from tests import chain_ref as CR

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def lib():
    from hevc_amd import _lib
    L = _lib.load()
    assert L.mihevc_device_count() >= 1, "no gfx950 device visible: the GPU tests need an MI355X"
    return L


def drain(enc):
    enc.flush()
    got = list(enc.packets())
    return b"".join(d for d, _, _ in got), [p for _, p, _ in got]


def cfg_of(depth, size, qp=None):
    cfg = K.cfg_of(depth, size)
    if qp is not None:
        cfg.qp = qp
    return cfg


@functools.lru_cache(maxsize=None)
def plain_stream(name, depth, out_depth=None, n=K.N_FRAMES, without=None, qp=None):
    """(stream, pts list) of a session fed the model's pictures of a case through mihevc_send_frame; without: the model of the chain less that stage; qp: of
    both kinds of session, None for the common configuration's"""
    from hevc_amd.encoder import Encoder
    case = case_of(name)
    chain = CR.without(case[2], without) if without else None
    pictures = K.model(case, depth, out_depth, n, chain)
    h, w = pictures[0][1][0].shape
    with Encoder(cfg_of(out_depth or depth, (w, h), qp), device=0) as enc:
        for pts, (y, u, v) in pictures:
            enc.send(np.ascontiguousarray(y), np.ascontiguousarray(u), np.ascontiguousarray(v), pts=pts)
        return drain(enc)


def case_of(name):
    return K.FULL if name == "full" else K.ONE_SLOT[name] if name in K.ONE_SLOT else K.TWO_SLOT[name]


def chain_stream(name, depth, out_depth=None, n=K.N_FRAMES, route="sync", check=None, qp=None):
    """(stream, pts list) of a session with the case's chain fed the case's clip; check(enc, i): called after frame i, and with None after the flush"""
    from hevc_amd.encoder import Encoder
    kind, size, chain = case_of(name)
    with Encoder(cfg_of(out_depth or depth, K.session_size((kind, size, chain)), qp), device=0) as enc:
        enc.set_chain(*size, depth, **K.lib_kwargs(chain))
        for i, f in enumerate(K.clip(kind, size, depth, n)):
            enc.send_chain(*f, asynchronous=route == "async")
            if check:
                check(enc, i)
        got = drain(enc)
        if check:
            check(enc, None)
        return got


# ------------------------------------------------------------------------------------------------ 1. one slot: the chain is the filter's own entry
def own_entry(enc, name, size, frame, depth):
    if name.startswith("deint"):
        enc.send_deint(*frame, tff=True, field_rate=name == "deint-field")
    elif name in ("ivtc", "match"):
        enc.send_fieldmatch(*frame, tff=True, decimate=name == "ivtc")
    elif name == "denoise":
        enc.send_denoise(*frame, strength=2)
    elif name == "scale":
        enc.send_scaled(*size, *frame, bit_depth=depth)
    elif name == "upscale":
        enc.send_upscaled(*size, *frame, bit_depth=depth, sharpen=8, antiring=8)
    else:
        enc.send_interpolate(*frame, factor=2)


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("name", sorted(K.ONE_SLOT))
def test_one_slot_chain_equals_the_entry_and_the_model(lib, name, depth):
    from hevc_amd.encoder import Encoder
    kind, size, chain = K.ONE_SLOT[name]
    want = plain_stream(name, depth)
    with Encoder(K.cfg_of(depth), device=0) as enc:
        for f in K.clip(kind, size, depth):
            own_entry(enc, name, size, f, depth)
        entry = drain(enc)
    got = chain_stream(name, depth)
    assert len(want[0]) > 200 and got == want and got == entry
    assert got[1] == list(range(CR.plan(chain, size + (depth,), K.SESSION + (depth,))["pictures"](K.N_FRAMES)))


# ------------------------------------------------------------------------------------------------ 2, 3. two slots, and all four
@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("name", sorted(K.MULTI))
def test_chain_stream_equals_the_model_fed_session(lib, name, depth):
    kind, size, chain = K.MULTI[name]
    want = plain_stream(name, depth)
    plan = CR.plan(chain, size + (depth,), K.SESSION + (depth,))
    decimates = chain.get("field") == "fieldmatch" and chain.get("decimate")

    def check(enc, i):
        if i is None:
            assert enc.stats().frames_in == plan["pictures"](K.N_FRAMES)
        elif decimates:          # a cycle's pictures leave the field stage with its fifth frame's successor
            assert enc.fieldmatch_info(i) is None

    got = chain_stream(name, depth, check=check)
    assert len(want[0]) > 200 and got == want
    assert got[1] == list(range(plan["pictures"](K.N_FRAMES)))
    for stage in CR.stages_on(chain):          # no stage is idle: without it the stream is another
        if stage == "resize":
            assert K.model(K.MULTI[name], depth, chain=CR.without(chain, stage))[0][1][0].shape != K.model(K.MULTI[name], depth)[0][1][0].shape
        else:
            assert plain_stream(name, depth, without=stage) != want, stage


def test_fieldmatch_info_of_a_chain_tells_the_models_decisions(lib):
    decided = K.model(K.FULL, 8, with_plan=True)[1]

    def check(enc, i):
        if i is not None:
            return
        for k, d in enumerate(decided):
            f = enc.fieldmatch_info(k)
            got = (list(f.comb_sum) + list(f.comb_block) + [f.dup_sum, f.dup_block], f.match, f.deinterlaced, f.dropped, f.picture)
            assert got == (d["metrics"], d["match"], int(d["deinterlaced"]), int(d["dropped"]), d["picture"]), (k, got, d)

    assert chain_stream("full", 8, check=check) == plain_stream("full", 8)


# ------------------------------------------------------------------------------------------------ 4. an 8-bit source into a 10-bit session
def test_full_chain_from_8_bit_into_a_10_bit_session(lib):
    want = plain_stream("full", 8, 10)
    assert len(want[0]) > 200 and chain_stream("full", 8, 10) == want
    assert want != plain_stream("full", 10)


# ------------------------------------------------------------------------------------------------ 5. the network as the resize stage
SR_SCALE = 2          # compact, x2: 52x36 becomes 104x72, which the route of mihevc_send_frame_sr_yuv fits into the 100x68 session


def sr_cfg(depth):
    cfg = K.cfg_of(depth)
    cfg.matrix = 1
    return cfg


def test_denoise_then_sr_equals_the_sr_entry_fed_the_denoised_frames(lib):
    from hevc_amd.encoder import Encoder
    from tests import sr_compact_common as SC
    frames = K.clip("noisy", K.SMALL, 8, 5)
    denoised = CR.pictures(list(frames), 8, dict(denoise=2))
    with Encoder(sr_cfg(8), device=0) as enc:
        enc.set_sr_model(SC.session_model(SR_SCALE))
        for pts, p in denoised:
            enc.send_sr_yuv(*K.SMALL, *[np.ascontiguousarray(q) for q in p], bit_depth=8, matrix=6, pts=pts)
        want = drain(enc)
    with Encoder(sr_cfg(8), device=0) as enc:
        enc.set_sr_model(SC.session_model(SR_SCALE))
        enc.set_chain(*K.SMALL, 8, resize="sr", sr_matrix=6)
        for f in frames:
            enc.send_chain(*f)
        alone = drain(enc)
    with Encoder(sr_cfg(8), device=0) as enc:
        enc.set_sr_model(SC.session_model(SR_SCALE))
        enc.set_chain(*K.SMALL, 8, denoise=2, resize="sr", sr_matrix=6)
        for f in frames:
            enc.send_chain(*f)
        got = drain(enc)
    assert len(want[0]) > 200 and got == want and alone != want and alone[1] == want[1] == list(range(5))
    with Encoder(sr_cfg(8), device=0) as enc:          # the one-slot chain is the entry
        enc.set_sr_model(SC.session_model(SR_SCALE))
        for i, f in enumerate(frames):
            enc.send_sr_yuv(*K.SMALL, *f, bit_depth=8, matrix=6, pts=i)
        assert drain(enc) == alone


def test_sr_then_interpolate_equals_the_model_over_the_stage_entries(lib):
    """the pictures the interpolator gets are made by hand: mihevc_k_sr_compact_network over the model's R'G'B' of the frame, mihevc_k_convert_rgb to the 10-bit
    intermediate picture, mihevc_k_scale_source to the session's size; mcfi_ref.clip_pictures over them is fed through mihevc_send_frame"""
    from hevc_amd.encoder import Encoder
    from tests import mcfi_ref
    from tests import sr_compact_common as SC
    from tests import sr_yuv_common as Q
    from tests.test_gpu_scale import k_scale
    frames = K.clip("film", K.SMALL, 8, 4)
    W, H = K.SESSION
    model = SC.session_model(SR_SCALE)
    enlarged = []
    for f in frames:
        half = SC.network_planes(lib, model, *Q.rgb16_planes(f, 8, 6, False))
        enlarged.append(CR.crop(k_scale(lib, Q.intermediate_planes(lib, half, 1, False), 10, W, H, 8), W, H))
    pictures = [CR.crop(p, W, H) for p in mcfi_ref.clip_pictures(enlarged, 8, 2)]
    assert any(not np.array_equal(a[0], b[0]) for a, b in zip(pictures, mcfi_ref.clip_pictures(enlarged, 8, 2, 1)))          # a moving pair
    with Encoder(sr_cfg(8), device=0) as enc:
        for i, p in enumerate(pictures):
            enc.send(*[np.ascontiguousarray(q) for q in p], pts=i)
        want = drain(enc)
    with Encoder(sr_cfg(8), device=0) as enc:
        enc.set_sr_model(model)
        enc.set_chain(*K.SMALL, 8, resize="sr", sr_matrix=6, interpolate=2)
        for f in frames:
            enc.send_chain(*f)
        got = drain(enc)
    assert len(want[0]) > 200 and got == want and want[1] == list(range(7))


# ------------------------------------------------------------------------------------------------ 6. where the source lies
@pytest.fixture(scope="module")
def device_streams():
    """SHA-256 and pts of the streams of chain sessions fed from torch tensors, from ONE child process in which torch is initialised before the library
    (tests/chain_device_child.py says why)"""
    p = subprocess.run([sys.executable, "-s", "-m", "tests.chain_device_child"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    return json.loads(p.stdout[p.stdout.index("{"):])


@pytest.mark.parametrize("depth", [8, 10])
def test_sync_async_and_device_planes_give_one_stream(lib, device_streams, depth):
    want = plain_stream("full", depth)
    assert len(want[0]) > 200 and chain_stream("full", depth, route="async") == want and chain_stream("full", depth) == want
    assert device_streams[f"full-{depth}"] == [hashlib.sha256(want[0]).hexdigest(), want[1]]
    first = plain_stream("upscale-interp3", depth)          # a chain that begins with its resize stage: the planes are read where they lie
    assert device_streams[f"upscale-interp3-{depth}"] == [hashlib.sha256(first[0]).hexdigest(), first[1]]
    assert chain_stream("upscale-interp3", depth, route="async") == first


# ------------------------------------------------------------------------------------------------ 7, 8. short clips; flush with every ring pending
@pytest.mark.parametrize("n", [1, 2])
def test_short_clips(lib, n):
    """one frame: every stage's P = C = N, the interpolator gives its j = 0 picture; two: the pair's pictures and the last frame's.  QP 12, in both sessions:
    one picture of 100x68 has to make a stream of more than 200 bytes"""
    for name in ("full", "bob-interp2"):
        pictures = CR.plan(K.MULTI[name][2], K.MULTI[name][1] + (8,), K.SESSION + (8,))["pictures"](n)

        def check(enc, i):          # nothing leaves the full chain before the flush; field-rate frame 1 gives the two pictures of frame 0's first pair
            assert enc.stats().frames_in == (pictures if i is None else 0 if name == "full" or i == 0 else 2), (name, i)

        want = plain_stream(name, 8, n=n, qp=12)
        print(name, n, len(want[0]), "bytes")
        got = chain_stream(name, 8, n=n, check=check, qp=12)
        assert len(want[0]) > 200 and got == want and len(got[1]) == pictures


def test_flush_with_every_ring_pending(lib):
    """seven frames of the full chain: the first cycle has left the field stage (four pictures), three of them the denoiser and the resize stage; the
    interpolator has given the four pictures of two pairs.  At flush the field stage holds frame 6 undecided and frame 5's picture, the denoiser and the interpolator a
    frame each"""
    def check(enc, i):
        if i is not None:
            assert enc.stats().frames_in == (0 if i < 5 else 4), i
        else:
            assert enc.stats().frames_in == 11
    want = plain_stream("full", 8, n=7)
    assert chain_stream("full", 8, n=7, check=check) == want and want[1] == list(range(11))


# ------------------------------------------------------------------------------------------------ 9. refusals
def test_refusals_leave_the_session_coding_on(lib):
    from hevc_amd import _lib
    from hevc_amd.encoder import Encoder
    from tests import sr_compact_common as SC
    kind, size, chain = K.FULL
    frames = K.clip(kind, size, 8)
    desc = _lib.chain(*size, 8, **K.lib_kwargs(chain))
    p0 = [q.ctypes.data for q in frames[0]]
    sw = size[0]

    def send(enc, planes, py=sw, pc=sw // 2, pts=99, flags=0):
        return lib.mihevc_send_frame_chain(enc._s, *planes, py, pc, pts, flags)

    # set after a frame (of any entry); the plain session codes on
    model8 = K.model(K.ONE_SLOT["denoise"], 8)
    with Encoder(K.cfg_of(8), device=0) as enc:
        assert send(enc, p0) == _lib.ESTATE                                                     # no chain
        enc.send(*[np.ascontiguousarray(q) for q in model8[0][1]])
        assert lib.mihevc_set_source_chain(enc._s, C.byref(desc)) == _lib.ESTATE
        assert send(enc, p0) == _lib.ESTATE
        for pts, p in model8[1:]:
            enc.send(*[np.ascontiguousarray(q) for q in p])
        assert drain(enc) == plain_stream("denoise", 8)
    with Encoder(K.cfg_of(8), device=0) as enc:          # a ring entry's first frame has produced no picture yet: still a frame
        f = K.clip("noisy", K.SESSION, 8)
        enc.send_denoise(*f[0], strength=2)
        assert lib.mihevc_set_source_chain(enc._s, C.byref(_lib.chain(*K.SESSION, 8, denoise=2))) == _lib.ESTATE
        for g in f[1:]:
            enc.send_denoise(*g, strength=2)
        assert drain(enc) == plain_stream("denoise", 8)
    # a bad descriptor, a second set, bad frames, every other entry; the chain codes on
    with Encoder(K.cfg_of(8), device=0) as enc:
        assert lib.mihevc_set_source_chain(enc._s, None) == _lib.EINVAL
        assert lib.mihevc_set_source_chain(enc._s, C.byref(_lib.chain(*size, 8))) == _lib.EINVAL
        assert lib.mihevc_set_source_chain(enc._s, C.byref(_lib.chain(*size, 8, denoise=2))) == _lib.EINVAL          # no resize stage: not the session's size
        assert lib.mihevc_set_source_chain(enc._s, C.byref(_lib.chain(*size, 8, resize="sr"))) == _lib.EINVAL         # sr without a model
        enc.set_lut3d(np.zeros((2, 2, 2, 3), np.uint16))          # (a table, so that the colour table's entry gets as far as the state)
        enc.set_chain(*size, 8, chain=desc)
        assert lib.mihevc_set_source_chain(enc._s, C.byref(desc)) == _lib.ESTATE
        for i, f in enumerate(frames):
            p = [q.ctypes.data for q in f]
            if i in (0, 3, 6):
                for k in range(3):
                    assert send(enc, [None if j == k else q for j, q in enumerate(p)]) == _lib.EINVAL
                assert send(enc, p, py=sw - 1) == _lib.EINVAL and send(enc, p, pc=sw // 2 - 1) == _lib.EINVAL and send(enc, p, flags=4) == _lib.EINVAL
                if i:
                    assert send(enc, p, pts=i - 1) == _lib.EINVAL                            # a pts that does not increase
                big = [np.zeros((68, 100), np.uint8)] * 3
                q = [b.ctypes.data for b in big]
                assert lib.mihevc_send_frame(enc._s, *q, 100, 50, 99) == _lib.ESTATE
                assert lib.mihevc_send_frame_async(enc._s, *q, 100, 50, 99) == _lib.ESTATE
                assert lib.mihevc_send_frame_device(enc._s, *q, 100, 50, 99) == _lib.ESTATE
                assert lib.mihevc_send_frame_fmt(enc._s, C.byref(_lib.SrcFormat(422, 0, 8, 0)), *q, 100, 50, 99, 0) == _lib.ESTATE
                assert lib.mihevc_send_frame_scaled(enc._s, C.byref(_lib.ScaleSrc(100, 68, 8)), *q, 100, 50, 99, 0) == _lib.ESTATE
                assert lib.mihevc_send_frame_upscaled(enc._s, C.byref(_lib.UpscaleSrc(100, 68, 8, 8, 8)), *q, 100, 50, 99, 0) == _lib.ESTATE
                assert lib.mihevc_send_frame_deint(enc._s, C.byref(_lib.Deint(1, 0)), *q, 100, 50, 99, 0) == _lib.ESTATE
                assert lib.mihevc_send_frame_denoise(enc._s, C.byref(_lib.denoise_level(1)), *q, 100, 50, 99, 0) == _lib.ESTATE
                assert lib.mihevc_send_frame_fieldmatch(enc._s, C.byref(_lib.Fieldmatch(1, 1, 1)), *q, 100, 50, 99, 0) == _lib.ESTATE
                assert lib.mihevc_send_frame_interpolate(enc._s, C.byref(_lib.Interpolate(2, 0, 10)), *q, 100, 50, 99, 0) == _lib.ESTATE
                assert lib.mihevc_send_frame_rgb(enc._s, C.byref(_lib.rgb_format_for("gbrp")), *q, 100, 99, 0) == _lib.ESTATE
                ptrs = [(C.c_void_p * 1)(b) for b in q]
                assert lib.mihevc_send_frames_device(enc._s, 1, *ptrs, 100, 50, 99) == _lib.ESTATE
                assert lib.mihevc_send_frame_lut3d(enc._s, C.byref(_lib.Lut3dSrc(8, 1, 0)), *q, 100, 50, 99, 0) == _lib.ESTATE
            enc.send_chain(*f, pts=i)
        got = drain(enc)
        assert send(enc, p0, pts=1000) == _lib.ESTATE                                            # after flush
    assert got == plain_stream("full", 8)
    # sr: set once the model is there; a model dropped on the way refuses the frame, set again the chain goes on
    small = K.clip("noisy", K.SMALL, 8, 4)
    streams = []
    for drop in (False, True):
        with Encoder(sr_cfg(8), device=0) as enc:
            sr = _lib.chain(*K.SMALL, 8, resize="sr", sr_matrix=6)
            assert lib.mihevc_set_source_chain(enc._s, C.byref(sr)) == _lib.EINVAL
            enc.set_sr_model(SC.session_model(SR_SCALE))
            enc.set_chain(*K.SMALL, 8, chain=sr)
            for i, f in enumerate(small):
                if drop and i == 2:
                    enc.set_sr_model(None)
                    assert send(enc, [q.ctypes.data for q in f], py=K.SMALL[0], pc=K.SMALL[0] // 2) == _lib.EINVAL
                    enc.set_sr_model(SC.session_model(SR_SCALE))
                enc.send_chain(*f)
            streams.append(drain(enc))
    assert streams[0] == streams[1] and len(streams[0][0]) > 200
    # the three entries of the network, in a session that is exactly twice the source so that each of them gets as far as the state
    from tests import sr_common as S
    cfg = sr_cfg(8)
    cfg.width, cfg.height = 2 * K.SMALL[0], 2 * K.SMALL[1]
    both = []
    for chained in (True, False):
        with Encoder(cfg, device=0) as enc:
            enc.set_sr_model(SC.session_model(SR_SCALE))
            if chained:
                enc.set_chain(*K.SMALL, 8, resize="sr", sr_matrix=6)
            for i, f in enumerate(small):
                if chained and i == 1:
                    q = [b.ctypes.data for b in f]
                    rgb = [f[0].ctypes.data] * 3
                    fmt = S.session_format(8)
                    assert lib.mihevc_send_frame_sr_yuv(enc._s, C.byref(_lib.SrYuv(*K.SMALL, 8, 6, 0)), *q, K.SMALL[0], K.SMALL[0] // 2, 99, 0) == _lib.ESTATE
                    assert lib.mihevc_send_frame_sr(enc._s, C.byref(fmt), *K.SMALL, *rgb, K.SMALL[0], 99, 0) == _lib.ESTATE
                    assert lib.mihevc_send_frame_sr_fit(enc._s, C.byref(fmt), *K.SMALL, *rgb, K.SMALL[0], 99, 0) == _lib.ESTATE
                if chained:
                    enc.send_chain(*f)
                else:
                    enc.send_sr_yuv(*K.SMALL, *f, bit_depth=8, matrix=6)
            both.append(drain(enc))
    assert both[0] == both[1] and len(both[0][0]) > 200
    # a band of a picture coded as two slices takes no chain
    cfg = K.cfg_of(8)
    cfg.height = 64
    cfg.pic_height, cfg.slice_count, cfg.slice_index = 96, 2, 0
    cfg.slice_ctu_rows[0], cfg.slice_ctu_rows[1] = 2, 1
    cfg.rate_share_q16 = 43691
    with Encoder(cfg, device=0) as enc:
        assert lib.mihevc_set_source_chain(enc._s, C.byref(_lib.chain(100, 64, 8, denoise=2))) == _lib.EINVAL


# ------------------------------------------------------------------------------------------------ 10. encode_file(chain=...)
def mp4_track(path):
    """(timescale, duration) of the track's mdhd and the (count, delta) entries of its stts"""
    import struct
    from hevc_amd import mp4
    data = path.read_bytes()

    def inside(names, start=0, end=None):
        for name in names:
            _, start, end = [b for b in mp4.parse_boxes(data, start, len(data) if end is None else end) if b[0] == name][0]
        return start
    m = inside(("moov", "trak", "mdia", "mdhd"))
    timescale, duration = struct.unpack(">II", data[m + 12:m + 20])          # version 0: flags, creation, modification, then the two
    t = inside(("moov", "trak", "mdia", "minf", "stbl", "stts"))
    count = struct.unpack(">I", data[t + 4:t + 8])[0]
    return timescale, duration, [struct.unpack(">II", data[t + 8 + 8 * k:t + 16 + 8 * k]) for k in range(count)]


def test_encode_file_chain_on_a_y4m(lib, tmp_path, monkeypatch):
    """the full chain over a y4m file: the stream is the hand-fed chain session's of the same configuration, the track has the plan's rate and frame count"""
    from hevc_amd import encoder, mp4, probe, yuvio
    from tests.test_chain_cpu import mp4_samples
    kind, size, chain = K.FULL
    frames = K.clip(kind, size, 8)
    n = len(frames)
    src = tmp_path / "rip.y4m"
    yuvio.write_y4m(src, frames, *size, fps=30000 / 1001, interlace="t")
    seen, RealEncoder = [], encoder.Encoder

    class Keeping(RealEncoder):
        def __init__(self, cfg, device=0):
            super().__init__(cfg, device=device)
            self.stream = b""
            seen.append(self)

        def packets_dts(self):
            for data, pts, key, dts in super().packets_dts():
                self.stream += data
                yield data, pts, key, dts

    monkeypatch.setattr(encoder, "Encoder", Keeping)
    info = probe.VideoInfo(*size, 30000 / 1001, "", "", "", "yuv420p", "", "", 0, False, "eng", n, n * 1001 / 30000)
    out = tmp_path / "restored.mp4"
    assert encoder.encode_file(src, out, info, total_frames=n, device=0, chain=dict(deinterlace="ivtc", denoise=2, upscale=K.SESSION, interpolate=2)) == 0
    (enc,) = seen
    assert (enc.cfg.width, enc.cfg.height, enc.cfg.fps_num, enc.cfg.fps_den) == (*K.SESSION, 48000, 1001)
    assert mp4_samples(out) == 19 == CR.plan(chain, size + (8,), K.SESSION + (8,))["pictures"](n)
    # the track itself: 19 samples of 1001 ticks at 48000 ticks a second, 30000/1001 x 8/5
    rate = CR.plan(chain, size + (8,), K.SESSION + (8,))["rate"] * Fraction(30000, 1001)
    timescale, duration, stts = mp4_track(out)
    assert stts == [(19, rate.denominator)] and (timescale, duration) == (rate.numerator, 19 * rate.denominator) and rate == Fraction(48000, 1001)
    monkeypatch.setattr(encoder, "Encoder", RealEncoder)
    with RealEncoder(enc.cfg, device=0) as hand:
        hand.set_chain(*size, 8, **K.lib_kwargs(chain))
        for f in frames:
            hand.send_chain(*f)
        want = drain(hand)
    assert len(want[0]) > 200 and enc.stream == want[0]
