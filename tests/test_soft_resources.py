"""CPU: the soft-decision kernels (csrc/lora_metrics.hip k_soft_bits<SF>, csrc/lora_codec.hip
k_soft_chain_decode<RDD>) keep no scratch and spill nothing - code-object metadata of the built
library, read as tests/test_scan_resources.py reads it."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "lora-sdr-lightweight-standalone-library-_amd", "lora_phy_amd", "lib", "liblora_mi355x.so")


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    import kernel_resources

    if not os.path.exists(kernel_resources.READELF):
        pytest.skip("llvm-readelf not available")
    return kernel_resources.kernels(LIB)


def named(kernels, pattern):
    return {m.group(1): r for r in kernels for m in [re.search(pattern, r.get("demangled", r["name"]))] if m}


def assert_clean(r):
    assert r.get("private_segment_fixed_size", 0) == 0, r
    assert r.get("vgpr_spill_count", 0) == 0, r
    assert r.get("sgpr_spill_count", 0) == 0, r


def test_soft_bits_has_one_instance_per_sf_without_scratch_or_spills(kernels):
    ks = named(kernels, r"\bk_soft_bits<(\d+)>")
    assert sorted(ks, key=int) == [str(sf) for sf in range(6, 13)], sorted(ks)
    for r in ks.values():
        assert_clean(r)
        # 32 KiB of LDS a workgroup (dynamic): five of them fit a CU (20 waves), which needs <= 96 VGPRs
        assert r["vgpr_count"] <= 96, r["vgpr_count"]
        assert not r.get("group_segment_fixed_size"), r


def test_soft_decoder_has_one_instance_per_rdd_without_scratch_or_spills(kernels):
    ks = named(kernels, r"\bk_soft_chain_decode<(\d+)>")
    assert sorted(ks, key=int) == [str(r) for r in range(5)], sorted(ks)
    for r in ks.values():
        assert_clean(r)
        assert not r.get("group_segment_fixed_size"), r  # nothing is staged in LDS
