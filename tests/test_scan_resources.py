"""CPU: the sliding-scan kernel (csrc/lora_scan.hip, k_detect_scan) keeps no scratch and spills
nothing - code-object metadata of the built library, read as tests/test_codec_resources.py
reads it."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "lora-sdr-lightweight-standalone-library-_amd", "lora_phy_amd", "lib", "liblora_mi355x.so")


@pytest.fixture(scope="module")
def scan_kernels():
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    import kernel_resources

    if not os.path.exists(kernel_resources.READELF):
        pytest.skip("llvm-readelf not available")
    return [r for r in kernel_resources.kernels(LIB) if re.search(r"\bk_detect_scan\b", r.get("demangled", r["name"]))]


def test_the_scan_is_one_kernel_of_the_library(scan_kernels):
    assert len(scan_kernels) == 1, scan_kernels


def test_scan_kernel_has_no_scratch_and_no_spills(scan_kernels):
    r = scan_kernels[0]
    assert r.get("private_segment_fixed_size", 0) == 0, r
    assert r.get("vgpr_spill_count", 0) == 0, r
    assert r.get("sgpr_spill_count", 0) == 0, r
    # the occupancy the LDS footprint allows (3 workgroups of 4 waves per CU) needs <= 128 VGPRs
    assert r["vgpr_count"] <= 128, r["vgpr_count"]
