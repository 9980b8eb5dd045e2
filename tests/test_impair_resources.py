"""CPU: the built library holds one impairment kernel per output format - complex64, cs16, cs8 and
cu8, the instances of the template k_impair<format> (csrc/lora_impair.hip) - and every one of
them uses no scratch, spills nothing and keeps no static LDS.  Code-object metadata only."""
import os
import re
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


def impair_kernels(kernel_resources):
    return [r for r in kernel_resources.kernels(LIB) if "k_impair" in r.get("demangled", r["name"])]


def test_there_is_a_kernel_per_format(kernel_resources):
    names = sorted(r["demangled"] for r in impair_kernels(kernel_resources))
    assert len(names) == 4 and len(set(names)) == 4, names
    for f in (0, 1, 2, 3):
        assert any(re.search(r"\bk_impair<%d>" % f, n) for n in names), (f, names)


def test_no_scratch_no_spills_no_lds(kernel_resources):
    rows = impair_kernels(kernel_resources)
    assert rows
    for r in rows:
        assert r.get("private_segment_fixed_size", 0) == 0, r
        assert r.get("vgpr_spill_count", 0) == 0, r
        assert r.get("sgpr_spill_count", 0) == 0, r
        assert r.get("group_segment_fixed_size", 0) == 0, r
