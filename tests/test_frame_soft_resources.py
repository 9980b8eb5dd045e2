"""CPU: the kernels of the soft path through the self-describing frame (csrc/lora_codec.hip
k_frame_decode_soft<SF>, csrc/lora_metrics.hip k_soft_bits_frame<SF>, the instances of k_soft_bits'
body with reduced columns) are in the built library, keep no scratch and spill nothing -
code-object metadata of the built library, read as tests/test_soft_resources.py reads it."""
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


def assert_clean(r):
    assert r.get("private_segment_fixed_size", 0) == 0, r
    assert r.get("vgpr_spill_count", 0) == 0, r
    assert r.get("sgpr_spill_count", 0) == 0, r


def test_frame_soft_bits_has_one_instance_per_sf_without_scratch_or_spills(kernels):
    ks = {m.group(1): r for r in kernels
          for m in [re.search(r"\bk_soft_bits_frame<(\d+)>", r.get("demangled", r["name"]))] if m}
    assert sorted(ks, key=int) == [str(sf) for sf in range(7, 13)], sorted(ks)  # SF6 has no header block
    for r in ks.values():
        assert_clean(r)
        # the same 32 KiB of dynamic LDS a workgroup and the same occupancy bound as k_soft_bits
        assert r["vgpr_count"] <= 96, r["vgpr_count"]
        assert not r.get("group_segment_fixed_size"), r


def test_frame_soft_decoder_has_one_instance_per_sf_without_scratch_spills_or_lds(kernels):
    """The coding rate is a run-time value of each frame inside the kernel (one decoder serves
    every rate); sf is the template parameter."""
    ks = {m.group(1): r for r in kernels
          for m in [re.search(r"\bk_frame_decode_soft<(\d+)>", r.get("demangled", r["name"]))] if m}
    assert sorted(ks, key=int) == [str(sf) for sf in range(7, 13)], sorted(ks)
    for r in ks.values():
        assert_clean(r)
        assert not r.get("group_segment_fixed_size"), r  # nothing is staged
        assert r["vgpr_count"] <= 128, r["vgpr_count"]
