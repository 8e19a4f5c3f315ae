"""CPU: the instances of k_mcfi_search, k_mcfi_field and k_mcfi_render (hevc_amd/csrc/kernels/mcfi.h) build for gfx950 without scratch, and their LDS and
registers let as many workgroups share a CU as their launch bounds ask: hipcc cross-compiles without a GPU and reports per-kernel resources with
-Rpass-analysis=kernel-resource-usage.  Each kernel is compiled alone, from a translation unit that holds nothing but its instantiations, with the flags of the
product's Makefile."""
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "hevc_amd" / "csrc"

# kernel -> (argument block, LDS image, program, workgroups per CU of the second launch bound: NT = 256 lanes are four waves, one per SIMD)
KERNELS = {"k_mcfi_search": ("McfiSearchArgs", "McfiSearchShared", "mcfi_search_program", 4), "k_mcfi_field": ("McfiFieldArgs", "McfiFieldShared", "mcfi_field_program", 4),
           "k_mcfi_render": ("McfiRenderArgs", "McfiRenderShared", "mcfi_render_program", 2)}


def unit(kernel):
    args, shared, program, per_cu = KERNELS[kernel]
    return f"""#include "kernels/mcfi.h"
using namespace mihevc;
template <typename T> __global__ __launch_bounds__(NT, {per_cu}) void {kernel}(const {args} a)
{{
    __shared__ __align__(16) {shared} s;
    GpuExec ex;
    {program}<T>(ex, s, a, (int)blockIdx.x);
}}
template __global__ void {kernel}<uint8_t>(const {args});
template __global__ void {kernel}<uint16_t>(const {args});
"""


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_kernel_has_no_scratch_and_fits_its_launch_bounds(kernel, tmp_path):
    args, _, _, per_cu = KERNELS[kernel]
    device = (CSRC / "device.hip").read_text()
    m = re.search(r"template <typename T> __global__ __launch_bounds__\(NT, %d\) void %s\(const %s a\)\n\{\n(.*?)\n\}\n" % (per_cu, kernel, args), device, re.S)
    assert m and m.group(1) in unit(kernel), f"the product's {kernel} is no longer the kernel compiled here"
    src = tmp_path / f"{kernel}_unit.hip"
    src.write_text(unit(kernel))
    flags = re.search(r"CXXFLAGS \?= (.*)", (CSRC / "Makefile").read_text()).group(1).split()
    p = subprocess.run(["/opt/rocm/bin/hipcc", *flags, "--offload-arch=gfx950", "-I", str(CSRC), "-Rpass-analysis=kernel-resource-usage", "-c", str(src),
                        "-o", str(tmp_path / f"{kernel}_unit.o")], capture_output=True, text=True, cwd=CSRC, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    blocks = [b for b in re.split(r"remark: [^\n]*Function Name: ", p.stderr)[1:] if kernel in b.split(" [")[0]]
    assert len(blocks) == 2, [b.split(" [")[0] for b in blocks]
    for b in blocks:
        name = b.split(" [")[0]
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        vgpr = int(re.search(r" VGPRs: (\d+)", b).group(1))
        agpr = int(re.search(r" AGPRs: (\d+)", b).group(1))
        lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
        print(f"{name}: {vgpr} VGPRs, {agpr} AGPRs, {lds} bytes of LDS, {scratch} bytes of scratch")
        assert scratch == 0, f"{name}: {scratch} bytes of scratch per lane ({vgpr} VGPRs)"
        assert per_cu * lds <= 160 * 1024, f"{name}: {lds} bytes of LDS"
        assert vgpr + agpr <= 512 // per_cu, f"{name}: {vgpr} VGPRs and {agpr} AGPRs: fewer than {per_cu} waves per SIMD"          # 512 per SIMD lane
