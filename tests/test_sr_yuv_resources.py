"""CPU: both instances of k_sr_from_yuv (hevc_amd/csrc/kernels/sr_yuv.h) build for gfx950 without scratch and without LDS, within the registers their launch
bounds allow: hipcc cross-compiles without a GPU and reports per-kernel resources with -Rpass-analysis=kernel-resource-usage.  The method is
tests/test_sr_resources.py's: the kernel is compiled alone, from a translation unit that holds nothing but its instantiations, with the flags of the product's
Makefile, and the product's kernel body must be the body compiled here."""
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "hevc_amd" / "csrc"
INSTANCES = ["uint16_t", "uint8_t"]

UNIT = """#include "kernels/sr_yuv.h"
using namespace mihevc;
template <typename TI> __global__ __launch_bounds__(NT) void k_sr_from_yuv(const SrYuvArgs a)
{
    GpuExec ex;
    sr_from_yuv_program<TI>(ex, a, (int)blockIdx.x);
}
""" + "".join(f"template __global__ void k_sr_from_yuv<{i}>(const SrYuvArgs);\n" for i in INSTANCES)


def test_kernel_has_no_scratch_no_lds_and_fits_its_launch_bounds(tmp_path):
    device = (CSRC / "device.hip").read_text()
    m = re.search(r"template <typename TI> __global__ __launch_bounds__\(NT\) void k_sr_from_yuv\(const SrYuvArgs a\)\n\{\n(.*?)\n\}\n", device, re.S)
    assert m and m.group(1) in UNIT, "the product's kernel is no longer the kernel compiled here"
    assert set(re.findall(r"k_sr_from_yuv<([^>]+)>\)", device)) == set(INSTANCES)
    src = tmp_path / "k_sr_yuv_unit.hip"
    src.write_text(UNIT)
    flags = re.search(r"CXXFLAGS \?= (.*)", (CSRC / "Makefile").read_text()).group(1).split()
    p = subprocess.run(["/opt/rocm/bin/hipcc", *flags, "--offload-arch=gfx950", "-I", str(CSRC), "-Rpass-analysis=kernel-resource-usage", "-c", str(src),
                        "-o", str(tmp_path / "k_sr_yuv_unit.o")], capture_output=True, text=True, cwd=CSRC, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    blocks = [b for b in re.split(r"remark: [^\n]*Function Name: ", p.stderr)[1:] if "k_sr_from_yuv" in b.split(" [")[0]]
    assert len(blocks) == len(INSTANCES), [b.split(" [")[0] for b in blocks]
    for b in blocks:
        name = b.split(" [")[0]
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        vgpr = int(re.search(r" VGPRs: (\d+)", b).group(1))
        agpr = int(re.search(r" AGPRs: (\d+)", b).group(1))
        lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
        print(f"{name}: {vgpr} VGPRs, {agpr} AGPRs, {lds} bytes of LDS, {scratch} bytes of scratch")
        assert scratch == 0, f"{name}: {scratch} bytes of scratch per lane ({vgpr} VGPRs)"
        assert lds == 0, f"{name}: {lds} bytes of LDS"
        assert vgpr + agpr <= 512, f"{name}: {vgpr} VGPRs and {agpr} AGPRs: NT = 256 lanes are four waves, one per SIMD of 512 registers a lane"
