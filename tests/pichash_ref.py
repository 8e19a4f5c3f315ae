"""Decoded picture hash (H.265 Annex D, SEI payloadType 132) restated in numpy from its definitions, and a small reader of the suffix SEI NAL
units that carry it.  Shared by tests/test_pichash_cpu.py and tests/test_gpu_pichash.py.

pictureData of a colour component: its samples in raster order over the coded size, one byte each at 8 bit, two bytes (low, then sample >> 8)
above 8 bit.  MD5 (hash_type 0) is RFC 1321 over pictureData; CRC (1) is the bit loop of crc_bitloop over pictureData and two zero bytes,
starting at 0xFFFF; checksum (2) sums (s & 0xFF) ^ mask (and (s >> 8) ^ mask above 8 bit), mask = (x & 0xFF) ^ (y & 0xFF) ^ (x >> 8) ^ (y >> 8),
modulo 2^32."""
import hashlib

import numpy as np

POLY = 0x1021
MD5, CRC, CHECKSUM = 0, 1, 2


def picture_data(plane, bit_depth: int) -> bytes:
    a = np.ascontiguousarray(plane)
    return a.astype(np.uint8).tobytes() if bit_depth <= 8 else a.astype("<u2").tobytes()


def crc_bitloop(data: bytes) -> int:
    """the literal definition: every bit of data + two zero bytes, most significant bit of each byte first"""
    crc = 0xFFFF
    for byte in bytes(data) + b"\x00\x00":
        for i in range(7, -1, -1):
            msb = (crc >> 15) & 1
            crc = (((crc << 1) + ((byte >> i) & 1)) & 0xFFFF) ^ (msb * POLY)
    return crc


def _byte_table():
    t = []
    for b in range(256):
        r = b << 8
        for _ in range(8):
            r = ((r << 1) & 0xFFFF) ^ (POLY if r & 0x8000 else 0)
        t.append(r)
    return t


TABLE = _byte_table()      # TABLE[b] = b x^16 mod P: the register's high byte shifted out


def crc_table(data: bytes) -> int:
    """the same register, a byte at a time: r <- (r x^8 + byte) mod P"""
    r = 0xFFFF
    for byte in bytes(data) + b"\x00\x00":
        r = TABLE[r >> 8] ^ ((r & 0xFF) << 8) ^ byte
    return r


def _mulmod(a: int, b: int) -> int:
    r = 0
    for i in range(15, -1, -1):
        r = ((r << 1) & 0xFFFF) ^ (POLY if r & 0x8000 else 0)
        if (b >> i) & 1:
            r ^= a
    return r


def _xpow8(n: int) -> int:
    """x^(8 n) mod P"""
    r, base = 1, 0x100
    while n:
        if n & 1:
            r = _mulmod(r, base)
        base = _mulmod(base, base)
        n >>= 1
    return r


def crc_fast(data: bytes, segments: int = 4096) -> int:
    """crc_table for large planes: zero bytes in front of the message do not change a zero-started register, so the message is cut into equal
    segments whose remainders run side by side in numpy, then combined (r = r_left x^(8 len) + r_right) and the start value added"""
    d = np.frombuffer(bytes(data), dtype=np.uint8)
    n = len(d)
    seg = max(1, -(-n // segments))
    padded = np.zeros(seg * segments, dtype=np.uint8)
    padded[seg * segments - n:] = d
    cols = padded.reshape(segments, seg)
    tab = np.array(TABLE, dtype=np.uint32)
    r = np.zeros(segments, dtype=np.uint32)
    for j in range(seg):
        r = tab[r >> 8] ^ ((r & 0xFF) << 8) ^ cols[:, j]
    step, acc = _xpow8(seg), 0
    for v in r.tolist():
        acc = _mulmod(acc, step) ^ v
    return _mulmod(_mulmod(0xFFFF, _xpow8(n)) ^ acc, POLY)      # (0xFFFF x^(8n) + M) x^16 mod P


def checksum(plane, bit_depth: int) -> int:
    s = np.asarray(plane).astype(np.int64)
    h, w = s.shape
    y, x = np.mgrid[0:h, 0:w]
    mask = (x & 0xFF) ^ (y & 0xFF) ^ (x >> 8) ^ (y >> 8)
    total = int(((s & 0xFF) ^ mask).sum())
    if bit_depth > 8:
        total += int(((s >> 8) ^ mask).sum())
    return total & 0xFFFFFFFF


def plane_hash(plane, bit_depth: int, hash_type: int):
    if hash_type == MD5:
        return hashlib.md5(picture_data(plane, bit_depth)).digest()
    if hash_type == CRC:
        return crc_fast(picture_data(plane, bit_depth))
    return checksum(plane, bit_depth)


def picture_hash(planes, bit_depth: int, hash_type: int):
    return [plane_hash(p, bit_depth, hash_type) for p in planes]


# ---- the SEI side
def nal_units(stream: bytes):
    """Annex-B byte stream -> [(nal_unit_type, nuh_temporal_id_plus1, the NAL unit's bytes without its start code)]"""
    out, i, n, starts = [], 0, len(stream), []
    while True:
        k = stream.find(b"\x00\x00\x01", i)
        if k < 0:
            break
        starts.append(k + 3)
        i = k + 3
    for a, nxt in zip(starts, starts[1:] + [n + 3]):
        nal = stream[a:nxt - 3].rstrip(b"\x00")      # (a NAL unit never ends in a zero byte: the leading zero of the next four-byte start code)
        out.append(((nal[0] >> 1) & 63, nal[1] & 7, nal))
    return out


def strip_hash_sei(stream: bytes):
    """the stream without its suffix SEI NAL units (type 40), and those units"""
    keep, hashes = [], []
    for t, _, nal in nal_units(stream):
        (hashes if t == 40 else keep).append(nal)
    return b"".join(b"\x00\x00\x00\x01" + x for x in keep), hashes


def rbsp(nal: bytes) -> bytes:
    out, zeros = bytearray(), 0
    for b in nal[2:]:
        if zeros >= 2 and b == 3:
            zeros = 0
            continue
        out.append(b)
        zeros = zeros + 1 if b == 0 else 0
    return bytes(out)


def parse_hash_sei(nal: bytes):
    """one suffix SEI NAL unit holding one decoded picture hash message -> (hash_type, [3 values], payloadSize); MD5 values as 16 bytes"""
    assert (nal[0] >> 1) & 63 == 40 and nal[1] & 7 == 1 and nal[0] & 0x81 == 0 and nal[1] >> 3 == 0
    b = rbsp(nal)
    i, ptype, psize = 0, 0, 0
    while b[i] == 0xFF:
        ptype += 255
        i += 1
    ptype += b[i]
    i += 1
    while b[i] == 0xFF:
        psize += 255
        i += 1
    psize += b[i]
    i += 1
    assert ptype == 132, ptype
    body = b[i:i + psize]
    assert b[i + psize:] == b"\x80", b[i + psize:]          # rbsp_trailing_bits: the message ends byte aligned
    kind = body[0]
    width = {MD5: 16, CRC: 2, CHECKSUM: 4}[kind]
    assert psize == 1 + 3 * width
    vals = [body[1 + width * c:1 + width * (c + 1)] for c in range(3)]
    if kind != MD5:
        vals = [int.from_bytes(v, "big") for v in vals]
    return kind, vals, psize
