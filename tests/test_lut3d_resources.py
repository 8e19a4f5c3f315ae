"""CPU: the four instances of k_lut3d (hevc_amd/csrc/kernels/lut3d.h; uint8 / uint16 sources x uint8 / uint16 outputs) build for gfx950 without scratch and without
LDS, and their registers let two workgroups share a CU, as the launch bounds ask: hipcc cross-compiles without a GPU and reports per-kernel resources with
-Rpass-analysis=kernel-resource-usage.  The kernel is compiled alone, from a translation unit that holds nothing but its instantiation, with the flags of the
product's Makefile.  Only the resource remarks are read."""
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "hevc_amd" / "csrc"

UNIT = """#include "kernels/lut3d.h"
using namespace mihevc;
template <typename TI, typename TO> __global__ __launch_bounds__(NT, 2) void k_lut3d(const Lut3dArgs a)
{
    GpuExec ex;
    lut3d_tile_program<TI, TO>(ex, a, (int)blockIdx.x);
}
template __global__ void k_lut3d<uint8_t, uint8_t>(const Lut3dArgs);
template __global__ void k_lut3d<uint8_t, uint16_t>(const Lut3dArgs);
template __global__ void k_lut3d<uint16_t, uint8_t>(const Lut3dArgs);
template __global__ void k_lut3d<uint16_t, uint16_t>(const Lut3dArgs);
"""
WORKGROUPS_PER_CU = 2          # the second launch bound: NT = 256 lanes are four waves, one per SIMD, so two workgroups are two waves per SIMD


def test_k_lut3d_has_no_scratch_and_fits_two_workgroups_per_cu(tmp_path):
    device = (CSRC / "device.hip").read_text()
    m = re.search(r"template <typename TI, typename TO> __global__ __launch_bounds__\(NT, 2\) void k_lut3d\(const Lut3dArgs a\)\n\{\n(.*?)\n\}\n", device, re.S)
    assert m and m.group(1) in UNIT, "the product's k_lut3d is no longer the kernel compiled here"
    src = tmp_path / "lut3d_unit.hip"
    src.write_text(UNIT)
    flags = re.search(r"CXXFLAGS \?= (.*)", (CSRC / "Makefile").read_text()).group(1).split()
    p = subprocess.run(["/opt/rocm/bin/hipcc", *flags, "--offload-arch=gfx950", "-I", str(CSRC), "-Rpass-analysis=kernel-resource-usage", "-c", str(src),
                        "-o", str(tmp_path / "lut3d_unit.o")], capture_output=True, text=True, cwd=CSRC, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    blocks = [b for b in re.split(r"remark: [^\n]*Function Name: ", p.stderr)[1:] if "k_lut3d" in b.split(" [")[0]]
    assert len(blocks) == 4, [b.split(" [")[0] for b in blocks]
    for b in blocks:
        name = b.split(" [")[0]
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        vgpr = int(re.search(r" VGPRs: (\d+)", b).group(1))
        agpr = int(re.search(r" AGPRs: (\d+)", b).group(1))
        lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
        print(f"{name}: {vgpr} VGPRs, {agpr} AGPRs, {lds} bytes of LDS, {scratch} bytes of scratch")
        assert scratch == 0, f"{name}: {scratch} bytes of scratch per lane ({vgpr} VGPRs)"
        assert lds == 0, f"{name}: {lds} bytes of LDS"
        assert vgpr + agpr <= 512 // WORKGROUPS_PER_CU, f"{name}: {vgpr} VGPRs and {agpr} AGPRs: fewer than two waves per SIMD"          # 512 per SIMD lane
