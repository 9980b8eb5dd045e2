"""CPU: the frame finder's kernel (csrc/lora_find.hip, k_find_frames) is in the built library,
keeps no scratch, spills nothing, and its LDS - all static: two tiles of one ballot word and 64
staged index values per 64 windows, and two of successors, the launch adds none - stays within 64 KiB.  The ABI's
extremes (SF 6-12, any osr, hop, W or capacity) do not change it: the tile is a constant of the
kernel.  Code-object metadata of the built library, read as tests/test_scan_resources.py and
tests/test_resample_resources.py read it."""
import os
import re
import subprocess
import sys
import tempfile

import pytest

from lora_phy_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "lora-sdr-lightweight-standalone-library-_amd", "lora_phy_amd", "lib", "liblora_mi355x.so")
KERNEL = "k_find_frames"
LDS_BYTES = 64 * 1024


@pytest.fixture(scope="module")
def kernel_resources():
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    import kernel_resources

    if not os.path.exists(kernel_resources.READELF):
        pytest.skip("llvm-readelf not available")
    return kernel_resources


@pytest.fixture(scope="module")
def find_kernels(kernel_resources):
    return [r for r in kernel_resources.kernels(LIB) if re.search(r"\b%s\b" % KERNEL, r.get("demangled", r["name"]))]


def test_the_finder_is_one_kernel_of_the_library(find_kernels):
    assert len(find_kernels) == 1, find_kernels


def test_finder_kernel_has_no_scratch_and_no_spills(find_kernels):
    r = find_kernels[0]
    assert r["private_segment_fixed_size"] == 0, r
    assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, r
    # a workgroup of 1024 lanes (16 waves, 4 per SIMD) needs <= 128 VGPRs to be launched at all
    assert r["vgpr_count"] <= 128, r["vgpr_count"]


def static_lds(kernel_resources):
    """.group_segment_fixed_size of the kernel: in a kernel's metadata entry the keys are sorted,
    so it is the last such line before the entry's .name."""
    for img in kernel_resources.code_objects(LIB):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(img)
            f.flush()
            notes = subprocess.run([kernel_resources.READELF, "--notes", f.name], capture_output=True,
                                   text=True).stdout
        m = re.search(r"^\s*\.name:\s+\S*%s\S*\s*$" % KERNEL, notes, flags=re.M)
        if m:
            sizes = re.findall(r"^\s*(?:- )?\.group_segment_fixed_size:\s+(\d+)\s*$", notes[:m.start()], flags=re.M)
            return int(sizes[-1])
    raise AssertionError("kernel not found")


def test_lds_fits_and_is_what_the_tile_needs(kernel_resources):
    static = static_lds(kernel_resources)
    dynamic = 0  # the launch requests none (csrc/lora_find.hip), whatever the arguments
    tile = _capi.FIND_TILE
    # three buffers of tile / 64 ballot words and tile uint16 index values, two of tile uint16
    # successors, and the row's count for the fill
    assert static == 3 * (tile // 64 * 8 + tile * 2) + 2 * tile * 2 + 8, static
    assert static + dynamic <= LDS_BYTES
