"""CPU: both instances of k_deint (hevc_amd/csrc/kernels/deint.h) build for gfx950 without scratch, and their LDS and registers let four workgroups share a CU,
as the launch bounds ask: hipcc cross-compiles without a GPU and reports per-kernel resources with -Rpass-analysis=kernel-resource-usage.  The kernel is
compiled alone, from a translation unit that holds nothing but its instantiation, with the flags of the product's Makefile."""
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "hevc_amd" / "csrc"

UNIT = """#include "kernels/deint.h"
using namespace mihevc;
template <typename T> __global__ __launch_bounds__(NT, 4) void k_deint(const DeintArgs a)
{
    __shared__ __align__(16) DeintShared s;
    GpuExec ex;
    deint_tile_program<T>(ex, s, a, (int)blockIdx.x);
}
template __global__ void k_deint<uint8_t>(const DeintArgs);
template __global__ void k_deint<uint16_t>(const DeintArgs);
"""


def test_k_deint_has_no_scratch_and_fits_four_workgroups_per_cu(tmp_path):
    device = (CSRC / "device.hip").read_text()
    m = re.search(r"template <typename T> __global__ __launch_bounds__\(NT, 4\) void k_deint\(const DeintArgs a\)\n\{\n(.*?)\n\}\n", device, re.S)
    assert m and m.group(1) in UNIT, "the product's k_deint is no longer the kernel compiled here"
    src = tmp_path / "deint_unit.hip"
    src.write_text(UNIT)
    flags = re.search(r"CXXFLAGS \?= (.*)", (CSRC / "Makefile").read_text()).group(1).split()
    p = subprocess.run(["/opt/rocm/bin/hipcc", *flags, "--offload-arch=gfx950", "-I", str(CSRC), "-Rpass-analysis=kernel-resource-usage", "-c", str(src),
                        "-o", str(tmp_path / "deint_unit.o")], capture_output=True, text=True, cwd=CSRC, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    blocks = [b for b in re.split(r"remark: [^\n]*Function Name: ", p.stderr)[1:] if "k_deint" in b.split(" [")[0]]
    assert len(blocks) == 2, [b.split(" [")[0] for b in blocks]
    for b in blocks:
        name = b.split(" [")[0]
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        vgpr = int(re.search(r" VGPRs: (\d+)", b).group(1))
        lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
        assert scratch == 0, f"{name}: {scratch} bytes of scratch per lane ({vgpr} VGPRs)"
        assert 4 * lds <= 160 * 1024, f"{name}: {lds} bytes of LDS"
        assert vgpr <= 128, f"{name}: {vgpr} VGPRs: fewer than four waves per SIMD"          # 512 per SIMD lane / 4 waves
