"""CPU: every instance of k_sr_conv and k_sr_input (hevc_amd/csrc/kernels/sr_conv.h) builds for gfx950 without scratch, and their LDS and registers (VGPRs and
AGPRs together) let as many workgroups share a CU as the launch bounds ask: hipcc cross-compiles without a GPU and reports per-kernel resources with
-Rpass-analysis=kernel-resource-usage.  The kernels are compiled alone, from a translation unit that holds nothing but their instantiations, with the flags of
the product's Makefile."""
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "hevc_amd" / "csrc"
PER_CU = 2          # the second launch bound of k_sr_conv (SR_PER_CU): NT = 256 lanes are four waves, one per SIMD
CONV_INSTANCES = ["64, 1, true", "32, 4, false", "64, 4, false", "192, 4, false", "64, 2, false", "96, 2, false", "128, 2, false", "160, 2, false"]
INPUT_INSTANCES = ["uint32_t, true", "uint16_t, true", "uint16_t, false", "uint8_t, false"]

UNIT = """#include "kernels/sr_conv.h"
using namespace mihevc;
static_assert(SR_PER_CU == %d, "the bound this test holds the kernel to");
template <int CIN, int NB, bool PLANAR> __global__ __launch_bounds__(NT, SR_PER_CU) void k_sr_conv(const SrConvArgs a)
{
    __shared__ __align__(16) SrShared<CIN> s;
    GpuExec ex;
    sr_conv_program<CIN, NB, PLANAR>(ex, s, a, (int)blockIdx.x);
}
template <typename TI, bool FLT> __global__ __launch_bounds__(NT) void k_sr_input(const SrInputArgs a)
{
    GpuExec ex;
    sr_input_program<TI, FLT>(ex, a, (int)blockIdx.x);
}
""" % PER_CU + "".join(f"template __global__ void k_sr_conv<{i}>(const SrConvArgs);\n" for i in CONV_INSTANCES) \
    + "".join(f"template __global__ void k_sr_input<{i}>(const SrInputArgs);\n" for i in INPUT_INSTANCES)


def test_kernels_have_no_scratch_and_fit_their_launch_bounds(tmp_path):
    device = (CSRC / "device.hip").read_text()
    for head in (r"template <int CIN, int NB, bool PLANAR> __global__ __launch_bounds__\(NT, SR_PER_CU\) void k_sr_conv\(const SrConvArgs a\)",
                 r"template <typename TI, bool FLT> __global__ __launch_bounds__\(NT\) void k_sr_input\(const SrInputArgs a\)"):
        m = re.search(head + r"\n\{\n(.*?)\n\}\n", device, re.S)
        assert m and m.group(1) in UNIT, "the product's kernel is no longer the kernel compiled here"
    launched = set(re.findall(r"k_sr_conv<([^>]+)>\)", device)) | set(re.findall(r"k_sr_input<([^>]+)>\)", device))
    assert launched == set(CONV_INSTANCES) | set(INPUT_INSTANCES), launched
    src = tmp_path / "k_sr_unit.hip"
    src.write_text(UNIT)
    flags = re.search(r"CXXFLAGS \?= (.*)", (CSRC / "Makefile").read_text()).group(1).split()
    p = subprocess.run(["/opt/rocm/bin/hipcc", *flags, "--offload-arch=gfx950", "-I", str(CSRC), "-Rpass-analysis=kernel-resource-usage", "-c", str(src),
                        "-o", str(tmp_path / "k_sr_unit.o")], capture_output=True, text=True, cwd=CSRC, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    blocks = [b for b in re.split(r"remark: [^\n]*Function Name: ", p.stderr)[1:] if "k_sr_" in b.split(" [")[0]]
    assert len(blocks) == len(CONV_INSTANCES) + len(INPUT_INSTANCES), [b.split(" [")[0] for b in blocks]
    for b in blocks:
        name = b.split(" [")[0]
        per_cu = PER_CU if "k_sr_conv" in name else 1
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        vgpr = int(re.search(r" VGPRs: (\d+)", b).group(1))
        agpr = int(re.search(r" AGPRs: (\d+)", b).group(1))
        lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
        print(f"{name}: {vgpr} VGPRs, {agpr} AGPRs, {lds} bytes of LDS, {scratch} bytes of scratch")
        assert scratch == 0, f"{name}: {scratch} bytes of scratch per lane ({vgpr} VGPRs)"
        assert per_cu * lds <= 160 * 1024, f"{name}: {lds} bytes of LDS"
        assert vgpr + agpr <= 512 // per_cu, f"{name}: {vgpr} VGPRs and {agpr} AGPRs: fewer than {per_cu} waves per SIMD"          # 512 per SIMD lane
