"""CPU: the rational-rate bank's kernel (csrc/lora_resample.hip, k_channelize_resample) is in the
built library, keeps no scratch, spills nothing, and its static plus dynamic LDS stays within
64 KiB at every extreme of the ABI's limits - code-object metadata of the built library, read as
tests/test_channel_resources.py reads the integer bank's, and the file header's geometry rule
restated."""
import os
import re
import subprocess
import sys
import tempfile

import pytest

from tests import resample_checker as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "lora-sdr-lightweight-standalone-library-_amd", "lora_phy_amd", "lib", "liblora_mi355x.so")
KERNEL = "k_channelize_resample"
LDS_BYTES = 64 * 1024


@pytest.fixture(scope="module")
def kernel_resources():
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    import kernel_resources

    if not os.path.exists(kernel_resources.READELF):
        pytest.skip("llvm-readelf not available")
    return kernel_resources


def test_the_kernel_has_no_scratch_and_no_spills(kernel_resources):
    rows = [r for r in kernel_resources.kernels(LIB) if KERNEL in r.get("demangled", r["name"])]
    assert len(rows) == 1, rows
    r = rows[0]
    assert r["private_segment_fixed_size"] == 0, r
    assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, r


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


def dynamic_lds(T, Li, D, C):
    """The launch's dynamic LDS: resample_geometry (csrc/lora_resample.hip), restated."""
    reach = rc.reach(T, Li, D)

    def entries(tile):
        return D * (tile + (reach - 1) // D)

    tile = 64
    while tile > 8 and C * entries(tile) > 8192:
        tile //= 2
    cg = min(C, 8192 // entries(tile))
    assert cg >= 1
    return cg * entries(tile) * 8


def test_lds_fits_at_the_extremes(kernel_resources):
    static = static_lds(kernel_resources)
    assert dynamic_lds(4096, 16, 256, 32) == 3 * 2304 * 8  # the issue's extreme: tile 8, passes of 3
    worst = 0
    for Li in range(1, 17):
        for D in sorted({Li, Li + 1, 2 * Li, 64, 255, 256} - set(range(Li))):
            top = min(4096, 512 * Li)  # the most taps the ABI takes at this interp
            for T in {1, Li, top - Li + 1, top}:
                for C in (1, 2, 3, 8, 31, 32):
                    worst = max(worst, dynamic_lds(T, Li, D, C))
    assert 0 < worst and static + worst <= LDS_BYTES, (static, worst)
