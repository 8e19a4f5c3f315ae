"""CPU: sign data hiding (mihevc_config.sign_hide).  The rule the kernels apply, restated here in numpy on the oracle's transform and quantiser,
against the kernel sources stepped with the switch on (tests/emu); whole pictures stepped with the switch on obey the parity rule in every coded
4x4 group, and their symbols, coded by the product's host coder, decode with the repository's decoder (oracle/hevc_dec.c infers the hidden signs)
to the stepped reconstruction; the host coder refuses a group that breaks the rule; the golden SDH streams (tests/golden/streams_sdh.json)."""
import ctypes as C
import importlib.util
import json
from pathlib import Path

import numpy as np
import pytest

from hevc_amd import _lib
from oracle import oracle as O
from tests import util
from tests.sdh_ref import hide_group, scan4, scan_idx  # noqa: F401  (the rule itself: tests/sdh_ref.py)

GOLDEN = Path(__file__).parent / "golden"
_spec = importlib.util.spec_from_file_location("make_sdh_goldens", GOLDEN / "make_sdh_goldens.py")
S = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(S)
WANT = json.loads((GOLDEN / "streams_sdh.json").read_text())

QUANT_SCALE = (26214, 23302, 20560, 18396, 16384, 14564)


def reference(res, log2n, qp, bd, intra, scan, dst=False):
    """K3 with sign data hiding on the oracle's primitives: levels and reconstructed residual of one block"""
    coef = O.fwd_transform(res, dst, bd)
    lv = O.quant(coef, qp, bd, intra).astype(np.int64)
    q = qp + 6 * (bd - 8)
    qbits = 14 + q // 6 + (15 - bd - log2n)
    n = 1 << log2n
    for gy in range(0, n, 4):
        for gx in range(0, n, 4):
            g = lv[gy:gy + 4, gx:gx + 4]
            hide_group(g, coef[gy:gy + 4, gx:gx + 4].astype(np.int64), scan, QUANT_SCALE[q % 6], qbits)
    lv16 = lv.astype(np.int16)
    rec = O.inv_transform(O.dequant(lv16, qp, bd), dst, bd) if lv.any() else np.zeros((n, n), np.int16)
    return lv16, rec


def residuals(log2n, bd, kind, count, seed):
    n, top = 1 << log2n, (1 << bd) - 1
    rng = np.random.default_rng(seed)
    if kind == "random":
        amp = rng.integers(1, top + 1, size=(count, 1, 1))
        return np.clip(np.round(rng.normal(0, 1, (count, n, n)) * amp / 3), -top, top).astype(np.int16)
    blocks = [np.full((n, n), top), np.full((n, n), -top), np.where((np.arange(n)[:, None] + np.arange(n)) % 2, top, -top)]
    while len(blocks) < count:
        blocks.append(rng.choice([-top, top], size=(n, n)) * (rng.random((n, n)) < rng.random()))
    return np.array(blocks[:count], np.int16)


def k3_grid():
    for log2n in (2, 3, 4, 5):
        for scan in (0, 1, 2):
            for bd in (8, 10):
                for qp in (0, 22, 37, 51):
                    for kind in ("random", "full"):
                        yield log2n, scan, bd, qp, kind


def k3_run(call, log2n, scan, bd, qp, kind, intra, dst=False):
    """-> number of levels sign hiding changed; asserts the entry point equals the numpy rule"""
    count = 8 if log2n == 5 else 24
    res = residuals(log2n, bd, kind, count, seed=log2n * 1000 + scan * 100 + qp + bd)
    n = 1 << log2n
    lvl, rec = np.zeros_like(res), np.zeros_like(res)
    call(res, lvl, rec, count, log2n, qp, bd, intra, dst, scan)
    changed = 0
    for b in range(count):
        wl, wr = reference(res[b], log2n, qp, bd, intra, scan, dst)
        assert np.array_equal(lvl[b], wl), f"block {b}: levels"
        assert np.array_equal(rec[b], wr), f"block {b}: reconstructed residual"
        changed += int((wl != O.quant(O.fwd_transform(res[b], dst, bd), qp, bd, intra)).sum())
        assert wl.shape == (n, n)
    return changed


@pytest.fixture(scope="module")
def emu():
    return util.StageApi(util.stepped_library(), "emu_", sign_hide=1)


def test_rule_restated_in_numpy_equals_the_stepped_k3(emu):
    """residual_pipeline's sign hiding phase (every TU size, 4x4 DCT in the chroma planes) == the numpy rule, bit for bit, levels and reconstruction;
    so does the 4x4 core (k_transform4_blocks' program) on DCT and DST-VII blocks"""
    f, f4 = emu.lib.emu_transform_sdh, emu.lib.emu_transform4_sdh

    def call(res, lvl, rec, count, log2n, qp, bd, intra, dst, scan):
        assert f(util.ptr(res), util.ptr(lvl), util.ptr(rec), count, log2n, qp, bd, intra, scan, 1) == 0

    def call4(res, lvl, rec, count, log2n, qp, bd, intra, dst, scan):
        assert log2n == 2 and f4(util.ptr(res), util.ptr(lvl), util.ptr(rec), count, qp, bd, intra, int(dst), scan, 1) == 0
    changed = changed4 = 0
    for i, (log2n, scan, bd, qp, kind) in enumerate(k3_grid()):
        changed += k3_run(call, log2n, scan, bd, qp, kind, intra=i % 2)
        if log2n == 2:
            changed4 += k3_run(call4, log2n, scan, bd, qp, kind, intra=i % 2)
            changed4 += k3_run(call4, log2n, scan, bd, qp, kind, intra=1, dst=True)          # the NxN trial's DST-VII luma blocks
    assert changed > 500            # the rule does change levels on this grid
    assert changed4 > 100


def test_stepped_k3_without_sign_hiding_is_plain_k3(emu):
    f = emu.lib.emu_transform_sdh
    for log2n in (2, 3, 4, 5):
        for bd, qp in ((8, 22), (10, 37)):
            res = residuals(log2n, bd, "random", 8, seed=log2n)
            lvl, rec = np.zeros_like(res), np.zeros_like(res)
            assert f(util.ptr(res), util.ptr(lvl), util.ptr(rec), len(res), log2n, qp, bd, 1, 1, 0) == 0
            for b in range(len(res)):
                c = O.fwd_transform(res[b], False, bd)
                assert np.array_equal(lvl[b], O.quant(c, qp, bd, True))
    f4 = emu.lib.emu_transform4_sdh
    for dst in (False, True):
        for bd, qp in ((8, 22), (10, 37), (8, 0), (10, 51)):
            for intra in (0, 1):
                res = residuals(2, bd, "random", 40, seed=bd + qp + 2 * dst + intra)
                lvl, rec = np.zeros_like(res), np.zeros_like(res)
                assert f4(util.ptr(res), util.ptr(lvl), util.ptr(rec), len(res), qp, bd, intra, int(dst), 0, 0) == 0
                for b in range(len(res)):
                    lv = O.quant(O.fwd_transform(res[b], dst, bd), qp, bd, bool(intra))
                    assert np.array_equal(lvl[b], lv)
                    assert np.array_equal(rec[b], O.inv_transform(O.dequant(lv, qp, bd), dst, bd) if lv.any() else np.zeros((4, 4), np.int16))


def groups_breaking_the_rule(a, bd):
    """every coded 4x4 group of an analysis whose levels break the sign data hiding parity (scan order from the CU records): list of (plane, x, y)"""
    bad = []
    cu = a.cu
    for pl, coef in enumerate((a.coef_y, a.coef_u, a.coef_v)):
        h, w = coef.shape
        for gy in range(0, h, 4):
            for gx in range(0, w, 4):
                g = coef[gy:gy + 4, gx:gx + 4]
                if not g.any():
                    continue
                ly, lx = (gy, gx) if pl == 0 else (2 * gy, 2 * gx)
                r = cu[ly // 8, lx // 8]
                intra, nxn, log2 = not (r["flags"] & 1), bool(r["flags"] & 16), int(r["log2_size"])
                if not intra:
                    scan = 0
                elif pl == 0:
                    scan = scan_idx(2, 0, int(r["intra_mode"][((ly // 4) & 1) * 2 + ((lx // 4) & 1)])) if nxn else scan_idx(log2, 0, int(r["intra_mode"][0]))
                else:
                    scan = scan_idx(2 if nxn else log2 - 1, 1, int(r["chroma_mode"]))
                L = [int(g[p // 4, p % 4]) for p in scan4(scan)]
                nz = [n for n in range(16) if L[n]]
                if nz[-1] - nz[0] > 3 and (sum(abs(v) for v in L) & 1) != int(L[nz[0]] < 0):
                    bad.append((pl, gx, gy))
    return bad


def hidden_groups(a):
    """number of coded 4x4 groups whose first and last levels are more than 3 diagonal scan positions apart (a lower bound of what is hidden)"""
    n = 0
    for coef in (a.coef_y, a.coef_u, a.coef_v):
        h, w = coef.shape
        for gy in range(0, h, 4):
            for gx in range(0, w, 4):
                L = [int(coef[gy + p // 4, gx + p % 4]) for p in scan4(0)]
                nz = [k for k in range(16) if L[k]]
                n += bool(nz) and nz[-1] - nz[0] > 3
    return n


# whole pictures: the stepped stage cases (tests/test_kernel_source_stepped.py CASES) and some envelope cases; IDR with NxN, P with rdo_cg and the
# intra second pass, a B picture
PICTURE_CASES = [pytest.param(*c, "synth", id="-".join(map(str, c))) for c in ((64, 64, 30, 8, 8), (96, 80, 22, 8, 8), (136, 72, 35, 8, 16), (72, 104, 26, 10, 8), (160, 96, 14, 8, 12))] + \
                [pytest.param(*c, id="-".join(map(str, c))) for c in util.ENVELOPE_STAGE_CASES[::4]]


@pytest.mark.parametrize("w,h,qp,bd,rng,content", PICTURE_CASES)
def test_stepped_pictures_obey_the_rule_and_decode_to_their_reconstruction(emu, w, h, qp, bd, rng, content):
    lib = _lib.load()
    cfg = _lib.default_config()
    cfg.width, cfg.height, cfg.bit_depth, cfg.me_range, cfg.qp, cfg.keyint, cfg.bframes = w, h, bd, rng, qp, 5, 1
    cfg.intra_nxn, cfg.intra_in_p, cfg.rdo_cg, cfg.pre_search, cfg.sign_hide = 1, 1, 5, int(content != "synth"), 1
    cfg.level_idc = 93
    srcs = [util.content_frame(content, h, w, seed=3, shift=(2 * i, i), bit_depth=bd) for i in range(3)]
    pics = S.stepped_pictures(emu, cfg, srcs, [0], qp)
    assert [st for _, st, _, _, _ in pics] == [2, 1, 0]
    buf = (C.c_uint8 * (1 << 16))()
    n = lib.mihevc_write_parameter_sets(C.byref(cfg), buf, len(buf))
    dec, info = O.decode(bytes(buf[:n]) + b"".join(p for _, _, p, _, _ in pics))
    hidden = 0
    for i, st, _, a, rec in pics:
        assert not groups_breaking_the_rule(a, bd), f"picture {i} (slice type {st})"
        assert dec[i].same(rec), f"display picture {i} (slice type {st}): decoded != stepped reconstruction"
        hidden += hidden_groups(a)
    assert hidden > 0


def test_decoder_sees_the_pps_flag():
    cfg = S.config("p96x80_8bit")
    lib = _lib.load()
    buf = (C.c_uint8 * (1 << 16))()
    for on in (0, 1):
        cfg.sign_hide = on
        n = lib.mihevc_write_parameter_sets(C.byref(cfg), buf, len(buf))
        assert n > 0
        L = O.lib()
        d = L.orc_dec_open()
        try:
            assert L.orc_dec_decode(d, bytes(buf[:n]), n) >= 0
            v = C.c_longlong()
            assert L.orc_dec_query(d, b"pps.sign_hiding", C.byref(v)) and v.value == on
        finally:
            L.orc_dec_close(d)
    cfg.sign_hide = 2
    assert lib.mihevc_write_parameter_sets(C.byref(cfg), buf, len(buf)) == _lib.EINVAL


def test_harness_without_sign_hiding_equals_the_oracle():
    """the harness steps the same kernels as tests/test_kernel_source_stepped.py: switched off, its pictures are the oracle's"""
    api = util.StageApi(util.stepped_library(), "emu_", sign_hide=0)
    for w, h, qp, bd in ((96, 80, 22, 8), (72, 104, 26, 10)):
        prm_i, prm_p = O.default_params(qp - 3, bd, 8), O.default_params(qp, bd, 8)
        prm_i.intra_nxn = 1
        prm_p.rdo_cg, prm_p.intra_in_p, prm_p.rdo_zero = 5, 1, 1
        srcs = [util.synth_frame(h, w, seed=3, shift=(2 * i, i), bit_depth=bd) for i in range(3)]
        want = util.run_pipeline(O, srcs, prm_i, prm_p, bd)
        ref = None
        for i, (src, (a, d, f, sp)) in enumerate(zip(srcs, want)):
            got = api.intra(src, prm_i) if i == 0 else api.inter(src, ref, prm_p)
            assert util.same_analysis(a, got), f"picture {i}: " + util.describe_diff(a, got)
            ref = f
        b = api.b(srcs[1], want[0][2], want[2][2], O.default_params(qp + 2, bd, 8))
        ob = O.analyze_b(srcs[1], want[0][2], want[2][2], O.default_params(qp + 2, bd, 8))
        assert util.same_analysis(ob, b)


def test_host_coder_refuses_a_group_that_breaks_the_rule(emu):
    lib = _lib.load()
    name = "p96x80_8bit"
    cfg = S.config(name)
    pics = S.case_pictures(name, emu)
    i, st, coded, a, _ = pics[0]
    buf = (C.c_uint8 * (4 << 20))()
    sao = np.zeros(((cfg.width + 31) // 32) * ((cfg.height + 31) // 32), O.SAO_DTYPE)
    cfg.sao = 0

    def code(coef_y):
        return lib.mihevc_encode_picture_host(C.byref(cfg), 2, 0, 24, util.ptr(a.cu), util.ptr(coef_y), util.ptr(a.coef_u), util.ptr(a.coef_v), util.ptr(sao), buf, len(buf))
    assert code(a.coef_y) > 0
    # one luma group with its first and last level more than 3 positions apart: flip the first level's sign
    for gy in range(0, a.coef_y.shape[0], 4):
        for gx in range(0, a.coef_y.shape[1], 4):
            r = a.cu[gy // 8, gx // 8]
            if r["flags"] & 16:
                continue
            scan = scan_idx(int(r["log2_size"]), 0, int(r["intra_mode"][0]))
            g = a.coef_y[gy:gy + 4, gx:gx + 4]
            L = [int(g[p // 4, p % 4]) for p in scan4(scan)]
            nz = [k for k in range(16) if L[k]]
            if nz and nz[-1] - nz[0] > 3:
                p = scan4(scan)[nz[0]]
                broken = a.coef_y.copy()
                broken[gy + p // 4, gx + p % 4] *= -1
                assert code(broken) == _lib.EINVAL
                msg = lib.mihevc_last_error(None).decode()
                assert "sign data hiding" in msg and f"CTU ({gx // 32}, {gy // 32}) plane 0" in msg and f"({gx}, {gy})" in msg, msg
                cfg.sign_hide = 0            # without the flag the same levels are an ordinary (if different) picture
                assert code(broken) > 0
                return
    pytest.fail("no group with a hidden sign in the IDR picture")


def test_fixture_covers_every_case():
    assert set(WANT) == set(S.CASES)


@pytest.mark.parametrize("name", sorted(S.CASES))
def test_stepped_kernels_and_host_coder_still_produce_the_golden_sdh_pictures(emu, name):
    pics = S.case_pictures(name, emu)
    got = S.summary(pics)
    assert got["bytes"] == WANT[name]["bytes"] and got["pictures"] == WANT[name]["pictures"], "re-bless tests/golden/streams_sdh.json in the same commit if intended"
    assert got["recon"] == WANT[name]["recon"]
    cfg, buf = S.config(name), (C.c_uint8 * (1 << 16))()
    n = _lib.load().mihevc_write_parameter_sets(C.byref(cfg), buf, len(buf))
    dec, info = O.decode(bytes(buf[:n]) + b"".join(p for _, _, p, _, _ in pics))
    assert [S.frame_hash(d) for d in dec] == WANT[name]["recon"]
    for i, st, _, a, _ in pics:
        assert not groups_breaking_the_rule(a, cfg.bit_depth), (name, i, st)


def test_config_for_and_defaults():
    from hevc_amd.encoder import config_for
    from hevc_amd.probe import VideoInfo
    assert _lib.default_config().sign_hide == 0
    info = VideoInfo(64, 64, 30.0, "bt709", "bt709", "bt709", "yuv420p", "", "", 0)
    assert config_for(info, 19, 2940, 3528, 90, "4.0", "main").sign_hide == 0
    assert config_for(info, 19, 2940, 3528, 90, "4.0", "main", sign_hide=1).sign_hide == 1
