"""CPU: the decoded picture hash (mihevc_config.pic_hash, H.265 Annex D payloadType 132).  The numpy reference of tests/pichash_ref.py against its
own definitions (known answers, the literal CRC bit loop); the kernel programs of hevc_amd/csrc/kernels/pichash.h stepped on the CPU (tests/emu)
against that reference; the host MD5 of mihevc_k_picture_hash against hashlib; the suffix SEI NAL unit mihevc_write_picture_hash_sei writes, read back;
configuration checks."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from hevc_amd import _lib
from tests import pichash_ref as R
from tests import util


@pytest.fixture(scope="module")
def emu():
    lib = util.stepped_library()
    lib.emu_picture_hash.argtypes = [C.c_void_p] * 3 + [C.c_int] * 5 + [C.c_void_p]
    return lib


def planes(w, h, bd, seed, fill=None):
    dt = np.uint8 if bd == 8 else np.uint16
    rng = np.random.default_rng(seed)
    shapes = [(h, w), (h // 2, w // 2), (h // 2, w // 2)]
    if fill is not None:
        return [np.full(s, fill, dt) for s in shapes]
    return [rng.integers(0, 1 << bd, s, dtype=np.int64).astype(dt) for s in shapes]


def emu_hash(emu, pl, bd, kind, order=0):
    out = np.zeros(3, np.uint32)
    h, w = pl[0].shape
    assert emu.emu_picture_hash(pl[0].ctypes.data, pl[1].ctypes.data, pl[2].ctypes.data, w, h, bd, kind, order, out.ctypes.data) == 0
    return [int(v) for v in out]


# ---- the reference against the definitions
def test_crc_known_answers():
    assert R.crc_bitloop(b"123456789") == 0xE5CC and R.crc_bitloop(b"") == 0x1D0F
    for f in (R.crc_table, R.crc_fast):
        assert f(b"123456789") == 0xE5CC and f(b"") == 0x1D0F


@pytest.mark.parametrize("bd", [8, 10])
def test_table_and_segmented_crc_equal_the_bit_loop(bd):
    for seed, (w, h) in enumerate([(16, 8), (40, 24), (64, 64)]):
        p = planes(w, h, bd, seed)[0]
        d = R.picture_data(p, bd)
        want = R.crc_bitloop(d)
        assert R.crc_table(d) == want and R.crc_fast(d) == want and R.crc_fast(d, segments=7) == want


def test_ten_bit_bytes_are_low_then_high():
    assert R.picture_data(np.array([[0x123, 0x3FF], [0, 0x100]], np.uint16), 10) == bytes([0x23, 0x01, 0xFF, 0x03, 0x00, 0x00, 0x00, 0x01])
    assert R.picture_data(np.array([[7, 255]], np.uint8), 8) == bytes([7, 255])


@pytest.mark.parametrize("bd", [8, 10])
def test_flat_planes_at_zero_and_maximum(bd):
    for fill in (0, (1 << bd) - 1):
        p = planes(48, 40, bd, 0, fill)[0]
        d = R.picture_data(p, bd)
        assert R.crc_fast(d) == R.crc_bitloop(d)
        lit = 0
        for y in range(40):
            for x in range(48):
                m = (x & 255) ^ (y & 255) ^ (x >> 8) ^ (y >> 8)
                lit += ((fill & 255) ^ m) + (((fill >> 8) ^ m) if bd > 8 else 0)
        assert R.checksum(p, bd) == lit & 0xFFFFFFFF


@pytest.mark.parametrize("bd", [8, 10])
def test_checksum_past_coordinate_255(bd):
    p = planes(520, 264, bd, 3)[0]
    lit = 0
    for y in range(264):
        for x in range(520):
            m = (x & 0xFF) ^ (y & 0xFF) ^ (x >> 8) ^ (y >> 8)
            s = int(p[y, x])
            lit += ((s & 0xFF) ^ m) + (((s >> 8) ^ m) if bd > 8 else 0)
    assert R.checksum(p, bd) == lit % (1 << 32)


# ---- the kernel programs stepped on the CPU
EMU_CASES = [(64, 64), (136, 72), (1920, 1080), (3840, 2160)]


@pytest.mark.parametrize("w,h", EMU_CASES, ids=[f"{w}x{h}" for w, h in EMU_CASES])
@pytest.mark.parametrize("bd", [8, 10])
def test_stepped_kernels_equal_reference(emu, w, h, bd):
    pl = planes(w, h, bd, w + h + bd)
    assert emu_hash(emu, pl, bd, 1) == R.picture_hash(pl, bd, R.CRC)
    assert emu_hash(emu, pl, bd, 2) == R.picture_hash(pl, bd, R.CHECKSUM)


@pytest.mark.parametrize("bd", [8, 10])
def test_stepped_kernels_any_thread_order_and_flat_planes(emu, bd):
    pl = planes(136, 72, bd, 11)
    for order in (1, 2):
        assert emu_hash(emu, pl, bd, 1, order) == R.picture_hash(pl, bd, R.CRC)
        assert emu_hash(emu, pl, bd, 2, order) == R.picture_hash(pl, bd, R.CHECKSUM)
    for fill in (0, (1 << bd) - 1):
        pl = planes(264, 136, bd, 0, fill)
        assert emu_hash(emu, pl, bd, 1) == R.picture_hash(pl, bd, R.CRC)
        assert emu_hash(emu, pl, bd, 2) == R.picture_hash(pl, bd, R.CHECKSUM)


# ---- host MD5 of the stage entry (no device needed for hash_type 0)
@pytest.mark.parametrize("w,h,bd", [(64, 64, 8), (136, 72, 10), (1920, 1080, 8)])
def test_host_md5_equals_hashlib(w, h, bd):
    pl = planes(w, h, bd, 5)
    out = (C.c_uint8 * 48)()
    assert _lib.load().mihevc_k_picture_hash(0, pl[0].ctypes.data, pl[1].ctypes.data, pl[2].ctypes.data, w, h, bd, 0, out) == 0
    got = bytes(out)
    assert [got[16 * c:16 * c + 16] for c in range(3)] == [hashlib.md5(R.picture_data(p, bd)).digest() for p in pl]


# ---- the SEI NAL unit
def write_sei(hash_type, values):
    lib = _lib.load()
    cfg = _lib.default_config()
    buf = (C.c_uint8 * 256)()
    if hash_type == R.MD5:
        raw = (C.c_uint8 * 48)(*b"".join(values))
    else:
        raw = (C.c_uint32 * 3)(*values)
    n = lib.mihevc_write_picture_hash_sei(C.byref(cfg), hash_type, raw, buf, 256)
    assert n > 0, n
    return bytes(buf[:n])


@pytest.mark.parametrize("hash_type", [R.MD5, R.CRC, R.CHECKSUM])
def test_sei_round_trip(hash_type):
    rng = np.random.default_rng(hash_type)
    if hash_type == R.MD5:
        cases = [[rng.bytes(16) for _ in range(3)], [bytes(16), b"\x00\x00\x01\x00\x00\x02\x00\x00\x03" + bytes(7), b"\xff" * 16]]
    elif hash_type == R.CRC:
        cases = [[int(v) for v in rng.integers(0, 1 << 16, 3)], [0, 0, 0], [0x0000, 0x0003, 0x0100]]
    else:
        cases = [[int(v) for v in rng.integers(0, 1 << 32, 3)], [0, 0x00000001, 0x00000300], [0xFFFFFFFF, 0x00000002, 0]]
    for values in cases:
        nal = write_sei(hash_type, values)
        assert nal[:4] == b"\x00\x00\x00\x01"
        units = R.nal_units(nal)
        assert len(units) == 1 and units[0][0] == 40 and units[0][1] == 1
        kind, got, psize = R.parse_hash_sei(units[0][2])
        assert kind == hash_type and got == values and psize == {R.MD5: 49, R.CRC: 7, R.CHECKSUM: 13}[hash_type]
        body = units[0][2][2:]
        assert all(not (body[i] == 0 and body[i + 1] == 0 and body[i + 2] <= 2) for i in range(len(body) - 2))   # emulation prevention holds
    zeros = write_sei(hash_type, [bytes(16)] * 3 if hash_type == R.MD5 else [0, 0, 0])
    assert b"\x00\x00\x03" in zeros[6:]                                                                     # and was needed


def test_sei_rejects_bad_arguments():
    lib = _lib.load()
    cfg = _lib.default_config()
    buf = (C.c_uint8 * 256)()
    vals = (C.c_uint32 * 3)(0x10000, 0, 0)
    assert lib.mihevc_write_picture_hash_sei(C.byref(cfg), 1, vals, buf, 256) == _lib.EINVAL       # a CRC has 16 bits
    assert lib.mihevc_write_picture_hash_sei(C.byref(cfg), 3, vals, buf, 256) == _lib.EINVAL
    assert lib.mihevc_write_picture_hash_sei(C.byref(cfg), 0, (C.c_uint8 * 48)(), buf, 10) == _lib.ENOMEM


# ---- configuration
def test_pic_hash_config_validation():
    lib = _lib.load()
    buf = (C.c_uint8 * 4096)()
    for v, ok in [(0, True), (1, True), (2, True), (3, True), (4, False), (-1, False), (255, False)]:
        cfg = _lib.default_config()
        cfg.pic_hash = v
        rc = lib.mihevc_write_parameter_sets(C.byref(cfg), buf, 4096)
        assert (rc > 0) == ok, (v, rc)
    cfg = _lib.default_config()
    cfg.height, cfg.pic_height, cfg.slice_count, cfg.slice_index = 544, 1080, 2, 0
    cfg.slice_ctu_rows[0], cfg.slice_ctu_rows[1] = 17, 17
    assert lib.mihevc_write_parameter_sets(C.byref(cfg), buf, 4096) > 0
    cfg.pic_hash = 2
    assert lib.mihevc_write_parameter_sets(C.byref(cfg), buf, 4096) == _lib.EINVAL


def test_pic_hash_does_not_touch_the_parameter_sets():
    lib = _lib.load()
    outs = []
    for v in (0, 1, 2, 3):
        cfg = _lib.default_config()
        cfg.pic_hash = v
        buf = (C.c_uint8 * 4096)()
        n = lib.mihevc_write_parameter_sets(C.byref(cfg), buf, 4096)
        outs.append(bytes(buf[:n]))
    assert outs[1:] == outs[:1] * 3


def test_config_for_passes_pic_hash_through():
    from hevc_amd import encoder
    from hevc_amd.probe import VideoInfo
    import inspect
    assert inspect.signature(encoder.config_for).parameters["pic_hash"].default == 0
    info = VideoInfo(1920, 1080, 30.0, "bt709", "bt709", "bt709", "yuv420p", "", "", 2)
    assert encoder.config_for(info, 19, 2940, 3528, 90, "4.0", "main").pic_hash == 0
    assert encoder.config_for(info, 19, 2940, 3528, 90, "4.0", "main", pic_hash=2).pic_hash == 2
