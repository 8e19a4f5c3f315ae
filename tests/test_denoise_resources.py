"""CPU: both instances of k_denoise (hevc_amd/csrc/kernels/denoise.h) build for gfx950 without scratch, and their LDS and registers let four workgroups share a CU,
as the launch bounds ask: hipcc cross-compiles without a GPU and reports per-kernel resources with -Rpass-analysis=kernel-resource-usage.  The kernel is
compiled alone, from a translation unit that holds nothing but its instantiation, with the flags of the product's Makefile."""
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "hevc_amd" / "csrc"

UNIT = """#include "kernels/denoise.h"
using namespace mihevc;
template <typename T> __global__ __launch_bounds__(NT, 4) void k_denoise(const DenoiseArgs a)
{
    __shared__ __align__(16) DenoiseShared s;
    GpuExec ex;
    denoise_tile_program<T>(ex, s, a, (int)blockIdx.x);
}
template __global__ void k_denoise<uint8_t>(const DenoiseArgs);
template __global__ void k_denoise<uint16_t>(const DenoiseArgs);
"""
WORKGROUPS_PER_CU = 4          # the second launch bound: NT = 256 lanes are four waves, one per SIMD, so four workgroups are four waves per SIMD


def test_k_denoise_has_no_scratch_and_fits_four_workgroups_per_cu(tmp_path):
    device = (CSRC / "device.hip").read_text()
    m = re.search(r"template <typename T> __global__ __launch_bounds__\(NT, 4\) void k_denoise\(const DenoiseArgs a\)\n\{\n(.*?)\n\}\n", device, re.S)
    assert m and m.group(1) in UNIT, "the product's k_denoise is no longer the kernel compiled here"
    src = tmp_path / "denoise_unit.hip"
    src.write_text(UNIT)
    flags = re.search(r"CXXFLAGS \?= (.*)", (CSRC / "Makefile").read_text()).group(1).split()
    p = subprocess.run(["/opt/rocm/bin/hipcc", *flags, "--offload-arch=gfx950", "-I", str(CSRC), "-Rpass-analysis=kernel-resource-usage", "-c", str(src),
                        "-o", str(tmp_path / "denoise_unit.o")], capture_output=True, text=True, cwd=CSRC, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    blocks = [b for b in re.split(r"remark: [^\n]*Function Name: ", p.stderr)[1:] if "k_denoise" in b.split(" [")[0]]
    assert len(blocks) == 2, [b.split(" [")[0] for b in blocks]
    for b in blocks:
        name = b.split(" [")[0]
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        vgpr = int(re.search(r" VGPRs: (\d+)", b).group(1))
        agpr = int(re.search(r" AGPRs: (\d+)", b).group(1))
        lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
        print(f"{name}: {vgpr} VGPRs, {agpr} AGPRs, {lds} bytes of LDS, {scratch} bytes of scratch")
        assert scratch == 0, f"{name}: {scratch} bytes of scratch per lane ({vgpr} VGPRs)"
        assert WORKGROUPS_PER_CU * lds <= 160 * 1024, f"{name}: {lds} bytes of LDS"
        assert vgpr + agpr <= 512 // WORKGROUPS_PER_CU, f"{name}: {vgpr} VGPRs and {agpr} AGPRs: fewer than four waves per SIMD"          # 512 per SIMD lane
