"""CPU: the down-converter bank's kernels (csrc/lora_channelize.hip, k_channelize) keep no
scratch and spill nothing - code-object metadata of the built library, read as
tests/test_scan_resources.py reads the scan kernel's."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "lora-sdr-lightweight-standalone-library-_amd", "lora_phy_amd", "lib", "liblora_mi355x.so")


@pytest.fixture(scope="module")
def channel_kernels():
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    import kernel_resources

    if not os.path.exists(kernel_resources.READELF):
        pytest.skip("llvm-readelf not available")
    return [r for r in kernel_resources.kernels(LIB) if "k_channelize" in r.get("demangled", r["name"])]


def test_the_library_has_a_channelizer_kernel(channel_kernels):
    assert len(channel_kernels) >= 1, channel_kernels


def test_channelizer_kernels_have_no_scratch_and_no_spills(channel_kernels):
    for r in channel_kernels:
        assert r.get("private_segment_fixed_size", 0) == 0, r
        assert r.get("vgpr_spill_count", 0) == 0, r
        assert r.get("sgpr_spill_count", 0) == 0, r
