"""CPU: the built library holds the propagation kernel k_propagate (csrc/lora_propagate.hip), once,
and it uses no scratch and spills nothing (its LDS is the staging of one path's samples and of the
table rows a tile can touch).  Code-object metadata only."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "lora-sdr-lightweight-standalone-library-_amd", "lora_phy_amd", "lib", "liblora_mi355x.so")


@pytest.fixture(scope="module")
def kernel_resources():
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    import kernel_resources

    if not os.path.exists(kernel_resources.READELF):
        pytest.skip("llvm-readelf not available")
    return kernel_resources


def propagate_kernels(kernel_resources):
    return [r for r in kernel_resources.kernels(LIB) if "k_propagate" in r.get("demangled", r["name"])]


def test_there_is_one_kernel(kernel_resources):
    names = [r["demangled"] for r in propagate_kernels(kernel_resources)]
    assert len(names) == 1 and names[0].startswith("k_propagate("), names


def test_no_scratch_no_spills(kernel_resources):
    rows = propagate_kernels(kernel_resources)
    assert rows
    for r in rows:
        assert r.get("private_segment_fixed_size", 0) == 0, r
        assert r.get("vgpr_spill_count", 0) == 0, r
        assert r.get("sgpr_spill_count", 0) == 0, r
