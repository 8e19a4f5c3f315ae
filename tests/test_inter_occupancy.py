"""CPU: k_inter_ctu<u8> holds 5 workgroups per CU.  Registers: the same hipcc -Rpass-analysis=kernel-resource-usage compile as
test_kernel_resources.py must report 96 VGPRs or fewer (5 waves per SIMD) and no scratch.  LDS: the dynamic size at me_range 15 comes from a
host build of the kernel source's own layout (kernels/inter.h inter_lds) and must let 5 workgroups share the CU's 160 KiB.  The motion-
compensation windows get there by overlaying ResidualShared's union behind the fractional search's exchange; the layout is checked for every
search range and both sample sizes: no window overlaps another, the search's share, or anything of InterShared outside the union."""
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "hevc_amd" / "csrc"
LDS_PER_CU = 160 * 1024

PROBE = r"""
#include <cstddef>
#include <cstdio>
#include "kernels/common.h"
#include "kernels/inter.h"
using namespace mihevc;
template <typename T> static void show(int R)
{
    const InterLds l = inter_lds<T>(R);
    const size_t lo = offsetof(InterShared<T>, rs) + offsetof(ResidualShared, scratch);
    printf("%d %d %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", (int)sizeof(T), R, sizeof(InterShared<T>), lo, lo + sizeof(ResidualShared::scratch),
           lo + 4 * (size_t)FRAC_SCRATCH, l.y, ((size_t)mc_win_y(R) * mc_win_y_stride(R) + 16) * sizeof(T), l.u,
           ((size_t)mc_win_c(R) * mc_win_c_stride(R) + 16) * sizeof(T), l.v, ((size_t)mc_win_c(R) * mc_win_c_stride(R) + 16) * sizeof(T), l.bytes);
}
int main()
{
    for (int R = 1; R <= MAX_RANGE; R++) { show<uint8_t>(R); show<uint16_t>(R); }
}
"""


@pytest.fixture(scope="module")
def layouts(tmp_path_factory):
    d = tmp_path_factory.mktemp("inter_lds")
    (d / "probe.cpp").write_text(PROBE)
    subprocess.run(["g++", "-std=c++17", "-O1", "-w", "-I", str(CSRC), "-o", str(d / "probe"), str(d / "probe.cpp")], check=True)
    out = subprocess.run([str(d / "probe")], capture_output=True, text=True, check=True).stdout
    rows = {}
    for line in out.splitlines():
        v = [int(x) for x in line.split()]
        rows[(v[0], v[1])] = dict(shared=v[2], lo=v[3], hi=v[4], frac_end=v[5], wins=[(v[6], v[7]), (v[8], v[9]), (v[10], v[11])], bytes=v[12])
    return rows


def test_windows_never_overlap_live_lds(layouts):
    for (size, R), l in layouts.items():
        outside = (l["shared"] + 15) & ~15
        spans = []
        for at, n in l["wins"]:
            assert at % 16 == 0, (size, R, at)
            assert (l["frac_end"] <= at and at + n <= l["hi"]) or at >= outside, (size, R, at, n)
            assert at + n <= l["bytes"], (size, R)
            spans.append((at, at + n))
        spans.sort()
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), (size, R, spans)


def test_five_workgroups_per_cu_by_lds_at_range_15(layouts):
    l = layouts[(1, 15)]
    assert 5 * l["bytes"] <= LDS_PER_CU, l["bytes"]
    assert all(l["frac_end"] <= at < l["hi"] for at, _ in l["wins"][:2])      # luma and Cb overlay the residual area


def test_k_inter_ctu_u8_registers_allow_five_waves_per_simd(tmp_path):
    flags = re.search(r"CXXFLAGS \?= (.*)", (CSRC / "Makefile").read_text()).group(1).split()
    p = subprocess.run(["/opt/rocm/bin/hipcc", *flags, "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage", "-c", str(CSRC / "device.hip"),
                        "-o", str(tmp_path / "device.o")], capture_output=True, text=True, cwd=CSRC, timeout=1200)
    assert p.returncode == 0, p.stderr[-2000:]
    blocks = {b.split(" [")[0].strip(): b for b in re.split(r"remark: [^\n]*Function Name: ", p.stderr)[1:]}
    names = [k for k in blocks if re.search(r"k_inter_ctuIh", k)]      # both variants: luma window inside rs.scratch or behind InterShared
    assert len(names) == 2, list(blocks)
    for n in names:
        vgpr = int(re.search(r" VGPRs: (\d+)", blocks[n]).group(1))
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blocks[n]).group(1))
        assert vgpr <= 96 and scratch == 0, (n, vgpr, scratch)
