"""CPU: the compact super-resolution path without a device.  1. k_sr_compact stepped (tests/emu/sr_compact.cpp) against the exact integer
convolutions of tests/sr_compact_ref.py, bit for bit, every shape at sizes below, at and above the tile, in every thread order and over random LDS images, with
everything the launch does not own coming back as it was; 2. the host side of csrc/sr_compact_net.h against its own statements; 3. the whole network stepped,
within the project's bound E <= 2 E_h + 2^-11, after showing on M64 alone that the bound sees every defect the cases exist for; 4. the stepped kernel under
AddressSanitizer as a stand-alone program; 5. the entries refuse bad arguments before any device call."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from hevc_amd import _lib
from tests import sr_compact_common as S
from tests import sr_compact_ref as R
from tests import util

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def emu():
    return util.stepped_library()


# ------------------------------------------------------------------------------------------------ 1. the convolution, exactly
def test_the_tile_is_the_one_the_cases_are_built_around(emu):
    v = [C.c_int() for _ in range(4)]
    emu.emu_sr_compact_tile(*map(C.byref, v))
    assert [x.value for x in v] == [S.TW, S.TH, 4, 256]
    assert S.TW * S.TH * 4 < 17 * 17 * S.TW * S.TH and 265 > 16 * S.TW and 261 > 16 * S.TH      # MANY_TILES has more tiles than workgroups


@pytest.mark.parametrize("order", [0, 1, 2])
@pytest.mark.parametrize("case_id", S.STEPPED_IDS)
def test_stepped_conv_is_exact(emu, case_id, order):
    """what the launch writes equals the integer convolution bit for bit.  (A launch owns its whole output tensor: the garbage it starts as must be gone, and the
    exact-size copies of the harness hold every access inside the tensors)"""
    out, want = S.run_conv(emu, "emu_", case_id, order=order, seed=17 * order + len(case_id))
    assert np.array_equal(out, want), np.argwhere(out != want)[:5]


@pytest.mark.parametrize("case_id", ["first-37x35", "trunk-37x35", "tail4-37x35", "tail2-37x35"])
def test_fewer_workgroups_walk_the_same_tiles(emu, case_id):
    """two and five workgroups over nine tiles: the loop a launch of more than 256 tiles runs on the device"""
    for nwg in (2, 5):
        out, want = S.run_conv(emu, "emu_", case_id, order=2, seed=nwg, nwg=nwg)
        assert np.array_equal(out, want), nwg


def test_the_exact_cases_reach_what_they_exist_for():
    for cid in S.STEPPED_IDS:
        facts = S.conv_data(cid)[8]
        if "tail" in cid:
            assert facts["base changes the half"] > 10, (cid, facts)
        else:
            assert facts["negative under a slope"] > 100 and facts["pixels with different slopes"] >= 16, (cid, facts)


# ------------------------------------------------------------------------------------------------ 2. the network description
def info(emu, scale, convs, sw, sh):
    count, nbytes, launches, off = C.c_ulonglong(), C.c_ulonglong(), C.c_int(), (C.c_ulonglong * 4)()
    rc = emu.emu_sr_compact_info(scale, convs, sw, sh, C.byref(count), C.byref(nbytes), C.byref(launches), off)
    return rc, count.value, nbytes.value, launches.value, list(off)


@pytest.mark.parametrize("scale", [4, 2])
@pytest.mark.parametrize("convs", [1, 16, 32, 64])
def test_count_bytes_and_launch_list_are_what_the_header_states(emu, scale, convs):
    rc, count, nbytes, launches, off = info(emu, scale, convs, 480, 270)
    assert rc == 0
    last = 3 * scale * scale
    assert count == 64 * 3 * 9 + 64 + 64 + convs * (64 * 64 * 9 + 64 + 64) + last * 64 * 9 + last == R.count(scale, convs)
    px = 480 * 270
    assert px * 32 * 2 % 256 == 0 and nbytes == px * (64 + 128 + 128 + 6 * scale * scale)
    assert off == [0, px * 64, px * 192, px * 320]
    rc, _, nb2, _, off2 = info(emu, scale, convs, 13, 21)          # a size whose buffers are rounded up to 256 bytes each
    r256 = lambda n: (n + 255) // 256 * 256
    assert nb2 == r256(273 * 64) + 2 * r256(273 * 128) + r256(273 * 6 * scale * scale) and off2[1] == r256(273 * 64)
    assert launches == convs + 2
    flat = np.zeros(count, np.float32)
    lst = (C.c_int * (6 * launches))()
    emu.emu_sr_compact_launch_list.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int]
    assert emu.emu_sr_compact_launch_list(scale, convs, util.ptr(flat), count, lst, launches) == launches
    got = [tuple(lst[6 * i:6 * i + 6]) for i in range(launches)]
    X, A, B, OUT = 0, 1, 2, 3
    want = [(0, X, A, 0, 32, 64)] + [(1 + i, (A, B)[i % 2], (B, A)[i % 2], 0, 64, 64) for i in range(convs)] + [(convs + 1, (A, B)[convs % 2], OUT, scale, 64, 48 if scale == 4 else 16)]
    assert got == want
    assert emu.emu_sr_compact_launch_list(scale, convs, util.ptr(flat), count - 1, lst, launches) == -3


def test_info_refuses_other_models(emu):
    for scale, convs in ((3, 16), (1, 16), (4, 0), (4, 65)):
        assert info(emu, scale, convs, 48, 32)[0] == -3


# ------------------------------------------------------------------------------------------------ 3. the whole network
@pytest.mark.parametrize("case", S.NET_CASES, ids=S.net_id)
def test_the_bound_sees_every_defect(case):
    """on M64 alone: each defect moves the output by more than four bounds, so a stepped or device run inside the bound has none of them"""
    _, _, e_h = S.net_models(case)
    bound = 2 * e_h + 2.0 ** -11
    moved = S.broken_networks(case)
    print(f"{S.net_id(case)}: E_h {e_h:.3e} bound {bound:.3e} " + "  ".join(f"{k}: {v / bound:.0f}x" for k, v in moved.items()))
    assert len(moved) == (7 if case[0] == 3 else 6)
    for name, v in moved.items():
        assert v > 4 * bound, (name, v, bound)


@pytest.mark.parametrize("case", S.NET_CASES, ids=S.net_id)
def test_stepped_network_is_within_twice_the_half_models_error(emu, case):
    dev = S.run_network(emu, "emu_", case, order=S.NET_CASES.index(case) % 3, seed=S.NET_CASES.index(case))
    e_h, e_dev, bound = S.network_errors(dev, case)
    print(f"{S.net_id(case)}: E_h {e_h:.3e}  E_stepped {e_dev:.3e}  bound {bound:.3e}")
    assert np.isfinite(dev.astype(np.float32)).all() and 0 < e_h
    assert e_dev <= bound


# ------------------------------------------------------------------------------------------------ 4. sanitizers
def test_stepped_kernel_under_address_sanitizer(tmp_path):
    """a stand-alone program (its own main, no python in the process): the packer, the launch list and the stepped kernel over tensors that end with their last
    element.  A read or write past one ends it with the sanitizer's report"""
    exe = tmp_path / "sr_compact_asan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-w", "-o", str(exe),
                    str(ROOT / "tests" / "emu" / "sr_compact.cpp"), str(ROOT / "tests" / "emu" / "sr.cpp"), str(ROOT / "tests" / "sr_compact_asan_main.cc")], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert p.stdout.strip().endswith("runs")


# ------------------------------------------------------------------------------------------------ 5. the entries without a device
def test_entries_validate_first():
    lib = _lib.load()
    no_device = _lib.ENODEV if lib.mihevc_device_count() == 0 else 0
    d, x, wt, bias, slopes, _, garbage, _, _ = S.conv_data("trunk-4x4")
    out = garbage.copy()
    args = [util.ptr(a) for a in (x, wt, bias, slopes)] + [None, util.ptr(out)]
    assert lib.mihevc_k_sr_compact_conv(0, C.byref(d), *args) == no_device
    for field, value in (("cin", 48), ("cin", 96), ("cin_real", 0), ("cin_real", 65), ("width", 0), ("height", 8193), ("tail", 2)):
        bad = _lib.SrCompactConvDesc.from_buffer_copy(bytes(d))
        setattr(bad, field, value)
        assert lib.mihevc_k_sr_compact_conv(0, C.byref(bad), *args) == _lib.EINVAL, field
    bad = _lib.SrCompactConvDesc.from_buffer_copy(bytes(d))
    bad.reserved[1] = 1
    assert lib.mihevc_k_sr_compact_conv(0, C.byref(bad), *args) == _lib.EINVAL
    for i in (0, 1, 2, 3, 5):          # every array a plain layer reads or writes
        assert lib.mihevc_k_sr_compact_conv(0, C.byref(d), *[None if j == i else a for j, a in enumerate(args)]) == _lib.EINVAL, i
    t, tx, twt, tbias, _, tbase, tgarbage, _, _ = S.conv_data("tail4-4x4")
    targs = [util.ptr(a) for a in (tx, twt, tbias)] + [None, util.ptr(tbase), util.ptr(tgarbage.copy())]
    assert lib.mihevc_k_sr_compact_conv(0, C.byref(t), *targs) == no_device
    assert lib.mihevc_k_sr_compact_conv(0, C.byref(t), *targs[:4], None, targs[5]) == _lib.EINVAL          # the tail needs its base
    for field, value in (("scale", 3), ("scale", 1), ("cin", 32)):
        bad = _lib.SrCompactConvDesc.from_buffer_copy(bytes(t))
        setattr(bad, field, value)
        assert lib.mihevc_k_sr_compact_conv(0, C.byref(bad), *targs) == _lib.EINVAL, field
    fmt = _lib.rgb_format_for("gbrp")
    planes, _ = S.net_source((12, 20))
    _, flat = S.net_weights(1, 4)
    o = np.zeros((3, 80, 48), np.uint16)
    p = [util.ptr(a) for a in planes]
    call = lambda model, count=flat.size, w=12, h=20, wts=util.ptr(flat): lib.mihevc_k_sr_compact_network(0, None if model is None else C.byref(model), wts, count, C.byref(fmt), w, h, *p, w, util.ptr(o))
    assert call(_lib.SrCompact(4, 1)) == no_device
    for model in (None, _lib.SrCompact(3, 1), _lib.SrCompact(4, 0), _lib.SrCompact(4, 65), _lib.SrCompact(2, 1), _lib.SrCompact(4, 2)):      # (the last two: another count)
        assert call(model) == _lib.EINVAL, model
    assert call(_lib.SrCompact(4, 1), count=flat.size - 1) == call(_lib.SrCompact(4, 1), count=flat.size + 1) == _lib.EINVAL
    assert call(_lib.SrCompact(4, 1), wts=None) == _lib.EINVAL
    assert call(_lib.SrCompact(4, 1), w=3) == call(_lib.SrCompact(4, 1), h=3) == _lib.EINVAL          # a side below 4
    bad_model = _lib.SrCompact(4, 1)
    bad_model.reserved[5] = 1
    assert call(bad_model) == _lib.EINVAL
    m = _lib.SrCompact(4, 1)
    assert lib.mihevc_set_sr_compact(None, C.byref(m), util.ptr(flat), flat.size) == _lib.EINVAL          # (with a session: tests/test_gpu_sr_compact.py)
