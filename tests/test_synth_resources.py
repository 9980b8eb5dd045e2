"""CPU: the built library holds one synthesis kernel per output format - complex64, cs16, cs8 and
cu8, the instances of the template k_synthesize<format> (csrc/lora_synth.hip) - and every one of
them uses no scratch and spills nothing, keeps no static LDS, and its dynamic LDS fits 64 KiB at
the ABI's extremes.  Code-object metadata only."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "lora-sdr-lightweight-standalone-library-_amd", "lora_phy_amd", "lib", "liblora_mi355x.so")
LDS_BYTES = 65536
TILE = 1024


@pytest.fixture(scope="module")
def kernel_resources():
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    import kernel_resources

    if not os.path.exists(kernel_resources.READELF):
        pytest.skip("llvm-readelf not available")
    return kernel_resources


def synth_kernels(kernel_resources):
    return [r for r in kernel_resources.kernels(LIB) if "k_synthesize" in r.get("demangled", r["name"])]


def test_there_is_a_kernel_per_format(kernel_resources):
    names = sorted(r["demangled"] for r in synth_kernels(kernel_resources))
    assert len(names) == 4 and len(set(names)) == 4, names
    for f in (0, 1, 2, 3):
        assert any(re.search(r"\bk_synthesize<%d>" % f, n) for n in names), (f, names)


def test_no_scratch_and_no_spills(kernel_resources):
    rows = synth_kernels(kernel_resources)
    assert rows
    for r in rows:
        assert r.get("private_segment_fixed_size", 0) == 0, r
        assert r.get("vgpr_spill_count", 0) == 0, r
        assert r.get("sgpr_spill_count", 0) == 0, r
        assert r.get("group_segment_fixed_size", 0) == 0, r


def dynamic_lds(ntaps: int, interp: int, channels: int, sample_bytes: int) -> int:
    """The launch's dynamic LDS, restated from csrc/lora_synth.hip: the tile's stored samples and
    a 16-byte line, the taps, and `cg` channels of an even `pitch` of 8-byte entries."""
    P = -(-ntaps // interp)
    pitch = ((TILE - 1) // interp + 1 + P + 1) & ~1
    fixed = TILE * sample_bytes + 16 + 4 * ntaps
    cg = min(channels, (LDS_BYTES - fixed) // (8 * pitch))
    assert cg >= 1, (ntaps, interp, channels)
    return fixed + cg * pitch * 8


def test_lds_fits_at_the_extremes():
    worst = 0
    for U in (1, 2, 3, 8, 63, 64):
        for T in (1, max(U - 1, 1), U, U + 1, 65, 511, 512):
            for C in (1, 2, 5, 31, 32):
                for sb in (8, 4, 2):
                    worst = max(worst, dynamic_lds(T, U, C, sb))
    assert 0 < worst <= LDS_BYTES
