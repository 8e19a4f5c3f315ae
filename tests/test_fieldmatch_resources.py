"""CPU: the kernels of inverse telecine (hevc_amd/csrc/kernels/fieldmatch.h) build for gfx950 without scratch, and the LDS and registers of both instances of
k_fm_metrics let four workgroups share a CU, as its launch bounds ask: hipcc cross-compiles without a GPU and reports per-kernel resources with
-Rpass-analysis=kernel-resource-usage.  The kernels are compiled alone, from a translation unit that holds nothing but their instantiations, with the flags of the
product's Makefile."""
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "hevc_amd" / "csrc"

UNIT = """#include "kernels/fieldmatch.h"
using namespace mihevc;
template <typename T> __global__ __launch_bounds__(NT, 4) void k_fm_metrics(const FmArgs a)
{
    __shared__ __align__(16) FmShared s;
    GpuExec ex;
    fm_metrics_program<T>(ex, s, a, (int)blockIdx.x);
}
__global__ __launch_bounds__(NT) void k_fm_fold(const unsigned long long *part, int n, unsigned long long *out)
{
    __shared__ __align__(16) FmShared s;
    GpuExec ex;
    fm_fold_program(ex, s, part, n, out);
}
template <typename T> __global__ __launch_bounds__(NT) void k_fm_weave(const DeintArgs a)
{
    GpuExec ex;
    fm_weave_program<T>(ex, a, (int)blockIdx.x);
}
template __global__ void k_fm_metrics<uint8_t>(const FmArgs);
template __global__ void k_fm_metrics<uint16_t>(const FmArgs);
template __global__ void k_fm_weave<uint8_t>(const DeintArgs);
template __global__ void k_fm_weave<uint16_t>(const DeintArgs);
"""


def test_fieldmatch_kernels_have_no_scratch_and_metrics_fits_four_workgroups_per_cu(tmp_path):
    device = (CSRC / "device.hip").read_text()
    for head in (r"template <typename T> __global__ __launch_bounds__\(NT, 4\) void k_fm_metrics\(const FmArgs a\)",
                 r"__global__ __launch_bounds__\(NT\) void k_fm_fold\(const unsigned long long \*part, int n, unsigned long long \*out\)",
                 r"template <typename T> __global__ __launch_bounds__\(NT\) void k_fm_weave\(const DeintArgs a\)"):
        m = re.search(head + r"\n\{\n(.*?)\n\}\n", device, re.S)
        assert m and m.group(0) in UNIT, f"the product's kernel is no longer the one compiled here: {head}"
    src = tmp_path / "fieldmatch_unit.hip"
    src.write_text(UNIT)
    flags = re.search(r"CXXFLAGS \?= (.*)", (CSRC / "Makefile").read_text()).group(1).split()
    p = subprocess.run(["/opt/rocm/bin/hipcc", *flags, "--offload-arch=gfx950", "-I", str(CSRC), "-Rpass-analysis=kernel-resource-usage", "-c", str(src),
                        "-o", str(tmp_path / "fieldmatch_unit.o")], capture_output=True, text=True, cwd=CSRC, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    blocks = [b for b in re.split(r"remark: [^\n]*Function Name: ", p.stderr)[1:] if "k_fm_" in b.split(" [")[0]]
    assert len(blocks) == 5, [b.split(" [")[0] for b in blocks]
    for b in blocks:
        name = b.split(" [")[0]
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        vgpr = int(re.search(r" VGPRs: (\d+)", b).group(1))
        lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
        print(f"{name}: {vgpr} VGPRs, {lds} bytes of LDS, {scratch} bytes of scratch")
        assert scratch == 0, f"{name}: {scratch} bytes of scratch per lane ({vgpr} VGPRs)"
        if "k_fm_metrics" in name:
            assert 4 * lds <= 160 * 1024, f"{name}: {lds} bytes of LDS"
            assert vgpr <= 128, f"{name}: {vgpr} VGPRs: fewer than four waves per SIMD"          # 512 per SIMD lane / 4 waves
