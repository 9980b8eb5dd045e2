"""CPU: the built library holds a kernel per sample format for each bank - complex64, cs16, cs8
and cu8 - and every one of them meets the conditions tests/test_channel_resources.py and
tests/test_resample_resources.py state: no scratch, no spills, and for the rational bank static
plus dynamic LDS within 64 KiB at the ABI's extremes.  Code-object metadata only.

The kernels' names: the integer bank's are the instances of the template k_channelize<format>.
The rational bank's complex64 kernel keeps its name, k_channelize_resample - the one kernel of
that name tests/test_resample_resources.py counts - and its integer formats are
k_channelize_raw_resample<format>, instances of the same body; every kernel of either bank has
"k_channelize" in its name, which is how tests/test_channel_resources.py selects them."""
import os
import re
import subprocess
import sys
import tempfile

import pytest

from tests.test_resample_resources import LDS_BYTES, dynamic_lds

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


def banks(kernel_resources):
    """(integer bank's kernels, rational bank's kernels) by name."""
    rows = [r for r in kernel_resources.kernels(LIB) if "k_channelize" in r.get("demangled", r["name"])]
    rational = [r for r in rows if "resample" in r.get("demangled", r["name"])]
    return [r for r in rows if r not in rational], rational


def test_each_bank_has_a_kernel_per_format(kernel_resources):
    integer, rational = banks(kernel_resources)
    assert len(integer) >= 4, integer
    assert len(rational) >= 4, rational
    names = sorted(r["demangled"] for r in integer + rational)
    assert len(set(names)) == len(names)
    for f in (0, 1, 2, 3):
        assert any(re.search(r"\bk_channelize<%d>" % f, n) for n in names), (f, names)
    for f in (1, 2, 3):
        assert any(re.search(r"\bk_channelize_raw_resample<%d>" % f, n) for n in names), (f, names)
    assert sum("k_channelize_resample" in n for n in names) == 1


def test_no_scratch_and_no_spills(kernel_resources):
    integer, rational = banks(kernel_resources)
    for r in integer + rational:
        assert r.get("private_segment_fixed_size", 0) == 0, r
        assert r.get("vgpr_spill_count", 0) == 0, r
        assert r.get("sgpr_spill_count", 0) == 0, r


def static_lds_by_kernel(kernel_resources):
    """{kernel symbol: .group_segment_fixed_size}: in a kernel's metadata entry the keys are sorted,
    so a kernel's figure is the last such line before its .name."""
    out = {}
    for img in kernel_resources.code_objects(LIB):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(img)
            f.flush()
            notes = subprocess.run([kernel_resources.READELF, "--notes", f.name], capture_output=True,
                                   text=True).stdout
        for m in re.finditer(r"^\s*\.name:\s+(\S*k_channelize\S*)\s*$", notes, flags=re.M):
            sizes = re.findall(r"^\s*(?:- )?\.group_segment_fixed_size:\s+(\d+)\s*$", notes[:m.start()], flags=re.M)
            out[m.group(1)] = int(sizes[-1])
    return out


def test_lds_fits_at_the_extremes(kernel_resources):
    """tests/test_resample_resources.py's sweep of the rational bank's limits, for each of its
    kernels; the integer bank's dynamic LDS is at most 8192 entries of 8 bytes by its geometry
    rule (csrc/lora_bank.h, channel_geometry), so its kernels may keep no static LDS."""
    integer, rational = banks(kernel_resources)
    static = static_lds_by_kernel(kernel_resources)
    worst = 0
    for Li in range(1, 17):
        for D in sorted({Li, Li + 1, 2 * Li, 64, 255, 256} - set(range(Li))):
            top = min(4096, 512 * Li)
            for T in {1, Li, top - Li + 1, top}:
                for C in (1, 2, 3, 8, 31, 32):
                    worst = max(worst, dynamic_lds(T, Li, D, C))
    assert 0 < worst <= LDS_BYTES
    for r in rational:
        assert static[r["name"]] + worst <= LDS_BYTES, (r, worst)
    for r in integer:
        assert static[r["name"]] == 0, r
