"""CPU: registers, scratch and occupancy of the inter kernels, beside tests/test_inter_occupancy.py -- the numbers tools/resource_usage.py prints, from
the same hipcc -Rpass-analysis=kernel-resource-usage compile of device.hip with the Makefile's flags.  The integer search has a form compiled for
me_range 15 and one that takes the range from its arguments, at both sample types: none of the four may spill or fall below 5 waves per SIMD (5
workgroups per CU), which the specialised form did when it was first tried (96 VGPRs and 16 bytes of scratch).  k_inter_ctu<uint8_t, *> keeps 5 without
scratch, k_inter_ctu<uint16_t, *> at least 4, k_inter_ctu_b the 5 (8 bit) and 4 (16 bit) it had.  "Occupancy" is the compiler's waves per SIMD for the
kernel's registers; a value above the one asked for is no loss, so the bounds are lower bounds."""
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "hevc_amd" / "csrc"


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """mangled kernel name -> (VGPRs, scratch bytes per lane, waves per SIMD)"""
    d = tmp_path_factory.mktemp("inter_resources")
    flags = re.search(r"CXXFLAGS \?= (.*)", (CSRC / "Makefile").read_text()).group(1).split()
    p = subprocess.run(["/opt/rocm/bin/hipcc", *flags, "--offload-arch=gfx950", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                        str(CSRC / "device.hip"), "-o", str(d / "device.o")], capture_output=True, text=True, cwd=CSRC, timeout=1200)
    assert p.returncode == 0, p.stderr[-2000:]
    out = {}
    for b in re.split(r"remark: [^\n]*Function Name: ", p.stderr)[1:]:
        def g(k):
            return int(re.search(re.escape(k) + r": (\d+)", b).group(1))
        out[b.split(" [")[0].strip()] = (g(" VGPRs"), g("ScratchSize [bytes/lane]"), g("Occupancy [waves/SIMD]"))
    return out


def pick(kernels, pattern, count):
    names = sorted(k for k in kernels if re.search(pattern, k))
    assert len(names) == count, (pattern, names)
    return [(n, *kernels[n]) for n in names]


def test_k_me_search_all_four_forms_no_scratch_five_workgroups(kernels):
    # k_me_search<T, RANGE>: T = h (uint8_t) / t (uint16_t), RANGE = 15 / 0
    for form in ("IhLi15E", "IhLi0E", "ItLi15E", "ItLi0E"):
        (name, vgpr, scratch, occ), = pick(kernels, r"k_me_search" + form, 1)
        assert scratch == 0 and occ >= 5 and vgpr <= 96, (name, vgpr, scratch, occ)


def test_k_inter_ctu_keeps_its_occupancy_at_both_sample_types(kernels):
    for name, vgpr, scratch, occ in pick(kernels, r"k_inter_ctuIhLb[01]E", 2):
        assert scratch == 0 and occ >= 5 and vgpr <= 96, (name, vgpr, scratch, occ)
    for name, vgpr, scratch, occ in pick(kernels, r"k_inter_ctuItLb[01]E", 2):
        assert scratch == 0 and occ >= 4 and vgpr <= 128, (name, vgpr, scratch, occ)


def test_k_inter_ctu_b_keeps_its_occupancy_at_both_sample_types(kernels):
    (name, vgpr, scratch, occ), = pick(kernels, r"k_inter_ctu_bIhE", 1)
    assert scratch == 0 and occ >= 5 and vgpr <= 96, (name, vgpr, scratch, occ)
    (name, vgpr, scratch, occ), = pick(kernels, r"k_inter_ctu_bItE", 1)
    assert scratch == 0 and occ >= 4 and vgpr <= 128, (name, vgpr, scratch, occ)
