"""CPU: the four instances of k_upscale (hevc_amd/csrc/kernels/upscale.h) build for gfx950 without scratch, and their LDS and registers let as many workgroups
share a CU as the launch bounds ask: hipcc cross-compiles without a GPU and reports per-kernel resources with -Rpass-analysis=kernel-resource-usage.  The kernel
is compiled alone, from a translation unit that holds nothing but its instantiations, with the flags of the product's Makefile."""
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "hevc_amd" / "csrc"
PER_CU = 8          # the second launch bound: NT = 256 lanes are four waves, one per SIMD

UNIT = """#include "kernels/upscale.h"
using namespace mihevc;
template <typename TI, typename TO> __global__ __launch_bounds__(NT, %d) void k_upscale(const UpscaleArgs a)
{
    __shared__ __align__(16) UpscaleShared s;
    GpuExec ex;
    upscale_tile_program<TI, TO>(ex, s, a, (int)blockIdx.x);
}
template __global__ void k_upscale<uint8_t, uint8_t>(const UpscaleArgs);
template __global__ void k_upscale<uint8_t, uint16_t>(const UpscaleArgs);
template __global__ void k_upscale<uint16_t, uint8_t>(const UpscaleArgs);
template __global__ void k_upscale<uint16_t, uint16_t>(const UpscaleArgs);
""" % PER_CU


def test_kernel_has_no_scratch_and_fits_its_launch_bounds(tmp_path):
    device = (CSRC / "device.hip").read_text()
    m = re.search(r"template <typename TI, typename TO> __global__ __launch_bounds__\(NT, %d\) void k_upscale\(const UpscaleArgs a\)\n\{\n(.*?)\n\}\n" % PER_CU, device, re.S)
    assert m and m.group(1) in UNIT, "the product's k_upscale is no longer the kernel compiled here"
    src = tmp_path / "k_upscale_unit.hip"
    src.write_text(UNIT)
    flags = re.search(r"CXXFLAGS \?= (.*)", (CSRC / "Makefile").read_text()).group(1).split()
    p = subprocess.run(["/opt/rocm/bin/hipcc", *flags, "--offload-arch=gfx950", "-I", str(CSRC), "-Rpass-analysis=kernel-resource-usage", "-c", str(src),
                        "-o", str(tmp_path / "k_upscale_unit.o")], capture_output=True, text=True, cwd=CSRC, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    blocks = [b for b in re.split(r"remark: [^\n]*Function Name: ", p.stderr)[1:] if "k_upscale" in b.split(" [")[0]]
    assert len(blocks) == 4, [b.split(" [")[0] for b in blocks]
    for b in blocks:
        name = b.split(" [")[0]
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        vgpr = int(re.search(r" VGPRs: (\d+)", b).group(1))
        agpr = int(re.search(r" AGPRs: (\d+)", b).group(1))
        lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
        print(f"{name}: {vgpr} VGPRs, {agpr} AGPRs, {lds} bytes of LDS, {scratch} bytes of scratch")
        assert scratch == 0, f"{name}: {scratch} bytes of scratch per lane ({vgpr} VGPRs)"
        assert PER_CU * lds <= 160 * 1024, f"{name}: {lds} bytes of LDS"
        assert vgpr + agpr <= 512 // PER_CU, f"{name}: {vgpr} VGPRs and {agpr} AGPRs: fewer than {PER_CU} waves per SIMD"          # 512 per SIMD lane
