"""CPU: tools/time_cabac.py codes the picture it says it codes.  A correctness test of the tool, no timing assertion: on a 128x64 picture its bytes are
those of mihevc_encode_picture_host called directly on the same symbols, from every thread and in every repeat, the access unit is one P slice with
residual in it, and the summary it prints has the fields DESIGN.md's tables quote."""
import ctypes as C
import importlib.util
import json
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("time_cabac", ROOT / "tools" / "time_cabac.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def picture(tool):
    return tool.Picture(128, 64, qp=27)


def test_bytes_equal_the_direct_call(tool, picture):
    times, data = picture.time(repeats=3, threads=2)
    assert len(times) == 6 and all(t > 0 for t in times)
    a, buf = picture.analysis, (C.c_uint8 * (1 << 20))()
    n = picture.lib.mihevc_encode_picture_host(C.byref(picture.cfg), 1, 1, picture.qp, a.cu.ctypes.data, a.coef_y.ctypes.data, a.coef_u.ctypes.data,
                                               a.coef_v.ctypes.data, picture.sao.ctypes.data, buf, len(buf))
    assert n > 0 and data == bytes(buf[:n])
    assert data[:4] == b"\x00\x00\x00\x01" and (data[4] >> 1) & 63 == 1      # one TRAIL_R slice NAL unit
    assert np.count_nonzero(a.coef_y) > 0, "the picture has no residual: the coder's level path would not run"


def test_summary_and_command_line(tool, capsys):
    s = tool.summary([0.003, 0.001, 0.002, 0.004])
    assert s == {"calls": 4, "median_ms": 2.5, "min_ms": 1.0, "max_ms": 4.0, "q1_ms": 1.25, "q3_ms": 3.75}
    assert tool.main(["--width", "128", "--height", "64", "--repeats", "2"]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["calls"] == 2 and line["threads"] == 1 and line["bytes"] > 0 and line["min_ms"] <= line["median_ms"] <= line["max_ms"]
