"""GPU (-m gpu): the decoded picture hash (mihevc_config.pic_hash) on an MI355X.  The CRC / checksum kernels alone (mihevc_k_picture_hash) against the
numpy reference of tests/pichash_ref.py; sessions with each hash kind carry one suffix SEI per access unit, behind its slice, whose values are the hash
of the picture the repository's decoder makes of the stream (taken without the SEI: the frozen readers do not know payloadType 132) and of the session's
own reconstruction; with aud = 0 the unstripped stream decodes; pic_hash = 0 changes nothing; the MP4 writer keeps the SEI."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from tests import pichash_ref as R
from tests import util

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from hevc_amd import _lib
    L = _lib.load()
    assert L.mihevc_device_count() >= 1, "no gfx950 device visible: the GPU tests need an MI355X"
    return L


def rand_planes(w, h, bd, seed):
    rng = np.random.default_rng(seed)
    dt = np.uint8 if bd == 8 else np.uint16
    return [rng.integers(0, 1 << bd, s, dtype=np.int64).astype(dt) for s in [(h, w), (h // 2, w // 2), (h // 2, w // 2)]]


def k_hash(lib, pl, bd, hash_type):
    h, w = pl[0].shape
    out = (C.c_uint8 * 48)()
    assert lib.mihevc_k_picture_hash(0, pl[0].ctypes.data, pl[1].ctypes.data, pl[2].ctypes.data, w, h, bd, hash_type, out) == 0
    raw = bytes(out)
    if hash_type == R.MD5:
        return [raw[16 * c:16 * c + 16] for c in range(3)]
    return [int.from_bytes(raw[4 * c:4 * c + 4], "little") for c in range(3)]


STAGE = [(64, 64, 8), (64, 64, 10), (136, 72, 8), (136, 72, 10), (1920, 1080, 8), (1920, 1080, 10), (3840, 2160, 8), (3840, 2160, 10)]


@pytest.mark.parametrize("w,h,bd", STAGE, ids=[f"{w}x{h}-{bd}" for w, h, bd in STAGE])
def test_stage_equals_reference(lib, w, h, bd):
    pl = rand_planes(w, h, bd, w * 7 + bd)
    for kind in (R.MD5, R.CRC, R.CHECKSUM):
        assert k_hash(lib, pl, bd, kind) == R.picture_hash(pl, bd, kind), f"hash_type {kind}"


def test_stage_8k_luma_and_flat_planes(lib):
    bd = 10
    pl = rand_planes(7680, 4320, bd, 1)
    for kind in (R.CRC, R.CHECKSUM):
        assert k_hash(lib, pl, bd, kind)[0] == R.plane_hash(pl[0], bd, kind)
    for fill in (0, 1023):
        pl = [np.full(p.shape, fill, np.uint16) for p in rand_planes(264, 136, bd, 0)]
        for kind in (R.CRC, R.CHECKSUM):
            assert k_hash(lib, pl, bd, kind) == R.picture_hash(pl, bd, kind)


# ---- sessions
def session_cfg(w, h, bd, bframes, pic_hash, aud=1):
    from hevc_amd import _lib
    cfg = _lib.default_config()
    cfg.width, cfg.height, cfg.bit_depth, cfg.keyint, cfg.min_keyint, cfg.scenecut, cfg.qp, cfg.me_range = w, h, bd, 30, 2, 0, 30, 12
    cfg.bframes, cfg.aud, cfg.gops_in_flight = bframes, aud, 1
    if bd == 10:      # Main10 HDR10 (core/utils.py:58-69)
        cfg.colour_primaries, cfg.transfer, cfg.matrix, cfg.hdr10, cfg.level_idc = 9, 16, 9, 1, 153
    if pic_hash is not None:
        cfg.pic_hash = pic_hash
    return cfg


def run_session(cfg, frames, bd, keep_recon=True):
    from hevc_amd.encoder import Encoder
    with Encoder(cfg, device=0, keep_recon=keep_recon) as enc:
        for f in frames:
            enc.send(*util.planes(f, bd))
        enc.flush()
        pk = list(enc.packets())
        recs = [enc.recon(i) for i in range(len(frames))] if keep_recon else None
    return pk, recs


def clip(w, h, bd, n):
    return [util.synth_frame(h, w, seed=4, shift=(2 * i, i), bit_depth=bd) for i in range(n)]


SESSIONS = [(1920, 1080, 8, 0, 4), (3840, 2160, 10, 1, 3)]


@pytest.mark.parametrize("w,h,bd,bframes,n", SESSIONS, ids=["1080p8", "2160p10-hdr-b"])
def test_session_hash_sei(lib, w, h, bd, bframes, n):
    frames = clip(w, h, bd, n)
    plain, _ = run_session(session_cfg(w, h, bd, bframes, 0), frames, bd, keep_recon=False)
    plain_stream = b"".join(p[0] for p in plain)
    dec, info = O.decode(plain_stream)
    assert len(dec) == n
    for pic_hash in (1, 2, 3):
        kind = pic_hash - 1
        pk, recs = run_session(session_cfg(w, h, bd, bframes, pic_hash), frames, bd)
        assert len(pk) == n
        want_dec = [R.picture_hash([d.y, d.u, d.v], bd, kind) for d in dec]
        for data, pts, _ in pk:
            units = R.nal_units(data)
            types = [t for t, _, _ in units]
            assert types.count(40) == 1, types
            last_vcl = max(i for i, t in enumerate(types) if t < 32)
            assert types.index(40) > last_vcl, types                      # behind the picture's slice
            got_kind, vals, _ = R.parse_hash_sei(units[types.index(40)][2])
            assert got_kind == kind
            assert vals == want_dec[pts], f"pic_hash {pic_hash}, picture {pts}: SEI != hash of the decoded picture"
            assert vals == R.picture_hash(recs[pts], bd, kind), f"pic_hash {pic_hash}, picture {pts}: SEI != hash of the reconstruction"
        stripped, seis = R.strip_hash_sei(b"".join(p[0] for p in pk))
        assert len(seis) == n
        assert stripped == R.strip_hash_sei(plain_stream)[0], "hashing changed the coded pictures"


def test_unstripped_stream_decodes_without_aud(lib):
    w, h, bd, n = 320, 192, 8, 5
    frames = clip(w, h, bd, n)
    pk, recs = run_session(session_cfg(w, h, bd, 0, 3, aud=0), frames, bd)
    stream = b"".join(p[0] for p in pk)
    dec, _ = O.decode(stream)
    assert len(dec) == n
    for i in range(n):
        assert dec[i].same(O.Frame(*recs[i]))
        assert R.parse_hash_sei(R.strip_hash_sei(pk[i][0])[1][0])[1] == R.picture_hash(recs[pk[i][1]], bd, R.CHECKSUM)
    from tests import hevc_syntax            # the independent syntax reader on the stream without its hash SEI
    stripped, seis = R.strip_hash_sei(stream)
    assert len(seis) == n and len(hevc_syntax.parse_stream(stripped).pictures) == n


def test_default_is_unchanged(lib):
    w, h, bd, n = 320, 192, 8, 5
    frames = clip(w, h, bd, n)
    a, _ = run_session(session_cfg(w, h, bd, 0, None), frames, bd, keep_recon=False)
    b, _ = run_session(session_cfg(w, h, bd, 0, 0), frames, bd, keep_recon=False)
    assert a == b
    assert not any(t == 40 for p in a for t, _, _ in R.nal_units(p[0]))


def test_mp4_keeps_the_hash_sei(lib, tmp_path):
    import struct
    from hevc_amd import mp4
    from hevc_amd.encoder import Encoder
    w, h, bd, n = 320, 192, 8, 5
    cfg = session_cfg(w, h, bd, 0, 2)
    path = tmp_path / "h.mp4"
    wr = mp4.Mp4Writer(path, cfg)
    with Encoder(cfg, device=0) as enc:
        for f in clip(w, h, bd, n):
            enc.send(*util.planes(f, bd))
        enc.flush()
        for data, pts, key, dts in enc.packets_dts():
            wr.add_sample(data, pts, key, dts)
        wr.finish(enc.headers())
    data = path.read_bytes()
    mdat = [(s, e) for kind, s, e in mp4.parse_boxes(data) if kind == "mdat"]
    assert len(mdat) == 1
    s, e = mdat[0]
    body = data[s:e]
    types, i = [], 0
    while i + 4 <= len(body):
        ln = struct.unpack(">I", body[i:i + 4])[0]
        types.append((body[i + 4] >> 1) & 63)
        i += 4 + ln
    assert types.count(40) == n and types.count(1) + types.count(19) + types.count(20) >= n
