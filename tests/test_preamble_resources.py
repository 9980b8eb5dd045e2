"""CPU: the kernels of preambled receive - k_detect_scan_acc (csrc/lora_scan.hip),
k_find_preamble and the shared k_select_frames (csrc/lora_find.hip) - keep no scratch and spill
nothing: code-object metadata of the built library, read as tests/test_scan_resources.py reads it."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "lora-sdr-lightweight-standalone-library-_amd", "lora_phy_amd", "lib", "liblora_mi355x.so")
KERNELS = ("k_detect_scan_acc", "k_find_preamble", "k_select_frames")


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    import kernel_resources

    if not os.path.exists(kernel_resources.READELF):
        pytest.skip("llvm-readelf not available")
    return kernel_resources.kernels(LIB)


@pytest.mark.parametrize("name", KERNELS)
def test_kernel_has_no_scratch_and_no_spills(kernels, name):
    found = [r for r in kernels if re.search(r"\b%s\b" % name, r.get("demangled", r["name"]))]
    assert len(found) == 1, found
    r = found[0]
    assert r.get("private_segment_fixed_size", 0) == 0, r
    assert r.get("vgpr_spill_count", 0) == 0, r
    assert r.get("sgpr_spill_count", 0) == 0, r
    if name == "k_detect_scan_acc":
        # the LDS footprint is k_detect_scan's, so the same occupancy needs <= 128 VGPRs
        assert r["vgpr_count"] <= 128, r["vgpr_count"]
