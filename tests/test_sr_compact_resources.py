"""CPU: every instance of k_sr_compact (hevc_amd/csrc/kernels/sr_compact.h) builds for gfx950 without scratch, and its LDS and registers (VGPRs and AGPRs
together) fit the launch bounds the header states (SRC_PER_CU workgroups of NT = 256 lanes per CU): hipcc cross-compiles without a GPU and reports per-kernel
resources with -Rpass-analysis=kernel-resource-usage.  The kernel is compiled alone, from a translation unit that holds nothing but its instantiations, with
the flags of the product's Makefile; the set of instances device.hip launches is the set compiled here."""
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "hevc_amd" / "csrc"
PER_CU = 1          # SRC_PER_CU
INSTANCES = ["64, 3, 4", "64, 1, 2", "32, 4, 0", "64, 4, 0"]
LDS = {"64, 3, 4": 55296 + 86016 + 512, "64, 1, 2": 18432 + 86016 + 512, "32, 4, 0": 36864 + 43008 + 512, "64, 4, 0": 73728 + 86016 + 512}      # weights + two tile images + parameters, as the header states

UNIT = """#include "kernels/sr_compact.h"
using namespace mihevc;
static_assert(SRC_PER_CU == %d, "the bound this test holds the kernel to");
template <int CIN, int NA, int TAIL> __global__ __launch_bounds__(NT, SRC_PER_CU) void k_sr_compact(const SrCompactArgs a)
{
    __shared__ __align__(16) SrCompactShared<CIN, NA> s;
    GpuExec ex;
    sr_compact_program<CIN, NA, TAIL>(ex, s, a, (int)blockIdx.x, (int)gridDim.x);
}
""" % PER_CU + "".join(f"template __global__ void k_sr_compact<{i}>(const SrCompactArgs);\n" for i in INSTANCES)


def test_kernels_have_no_scratch_and_fit_their_launch_bounds(tmp_path):
    device = (CSRC / "device.hip").read_text()
    head = r"template <int CIN, int NA, int TAIL> __global__ __launch_bounds__\(NT, SRC_PER_CU\) void k_sr_compact\(const SrCompactArgs a\)"
    m = re.search(head + r"\n\{\n(.*?)\n\}\n", device, re.S)
    assert m and m.group(1) in UNIT, "the product's kernel is no longer the kernel compiled here"
    launched = set(re.findall(r"k_sr_compact<([^>]+)>\)", device))
    assert launched == set(INSTANCES), launched
    src = tmp_path / "k_sr_compact_unit.hip"
    src.write_text(UNIT)
    flags = re.search(r"CXXFLAGS \?= (.*)", (CSRC / "Makefile").read_text()).group(1).split()
    p = subprocess.run(["/opt/rocm/bin/hipcc", *flags, "--offload-arch=gfx950", "-I", str(CSRC), "-Rpass-analysis=kernel-resource-usage", "-c", str(src),
                        "-o", str(tmp_path / "k_sr_compact_unit.o")], capture_output=True, text=True, cwd=CSRC, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    blocks = [b for b in re.split(r"remark: [^\n]*Function Name: ", p.stderr)[1:] if "k_sr_compact" in b.split(" [")[0]]
    assert len(blocks) == len(INSTANCES), [b.split(" [")[0] for b in blocks]
    seen = set()
    for b in blocks:
        name = b.split(" [")[0]
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        vgpr = int(re.search(r" VGPRs: (\d+)", b).group(1))
        agpr = int(re.search(r" AGPRs: (\d+)", b).group(1))
        lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
        print(f"{name}: {vgpr} VGPRs, {agpr} AGPRs, {lds} bytes of LDS, {scratch} bytes of scratch")
        assert scratch == 0, f"{name}: {scratch} bytes of scratch per lane ({vgpr} VGPRs)"
        assert lds in LDS.values() and PER_CU * lds <= 160 * 1024, f"{name}: {lds} bytes of LDS"
        seen.add(lds)
        assert vgpr + agpr <= 512 // PER_CU, f"{name}: {vgpr} VGPRs and {agpr} AGPRs"          # 512 per SIMD lane, one wave of the workgroup per SIMD
    assert seen == set(LDS.values())
