"""CPU: the self-describing frame's kernels (csrc/lora_codec.hip: k_frame_encode, k_frame_decode),
the frame gather (csrc/lora_gather.hip: k_gather_frames) and the two finder kernels
(csrc/lora_find.hip: k_find_candidates, k_select_frames) are in the built library, one instance
each, keep no scratch and spill nothing, and their LDS is static and what their source says,
whatever the arguments (the launches request no dynamic LDS).  Code-object metadata
of the built library, read as tests/test_find_resources.py reads it."""
import os
import re
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "lora-sdr-lightweight-standalone-library-_amd", "lora_phy_amd", "lib", "liblora_mi355x.so")
KERNELS = ("k_frame_encode", "k_frame_decode", "k_gather_frames", "k_find_candidates", "k_select_frames")
# static LDS: the codec and the gather stage nothing; the candidate kernel keeps a turn's 1024
# starts and two ballot words per wave, the pass a turn's 256 starts and symbol counts, four
# ballot words and its two carried values
LDS = {"k_frame_encode": 0, "k_frame_decode": 0, "k_gather_frames": 0,
       "k_find_candidates": 1024 * 8 + 2 * 16 * 8, "k_select_frames": 256 * 8 + 256 * 4 + 4 * 8 + 2 * 8}


@pytest.fixture(scope="module")
def kernel_resources():
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    import kernel_resources

    if not os.path.exists(kernel_resources.READELF):
        pytest.skip("llvm-readelf not available")
    return kernel_resources


@pytest.fixture(scope="module")
def by_kernel(kernel_resources):
    rows = kernel_resources.kernels(LIB)
    return {k: [r for r in rows if re.search(r"\b%s\b" % k, r.get("demangled", r["name"]))] for k in KERNELS}


@pytest.mark.parametrize("kernel", KERNELS)
def test_one_instance_without_scratch_or_spills(by_kernel, kernel):
    assert len(by_kernel[kernel]) == 1, by_kernel[kernel]
    r = by_kernel[kernel][0]
    assert r["private_segment_fixed_size"] == 0, r
    assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, r
    # a workgroup of 1024 lanes (the candidate kernel's) needs <= 128 VGPRs to be launched at all
    assert r["vgpr_count"] <= 128, r["vgpr_count"]


@pytest.mark.parametrize("kernel", KERNELS)
def test_static_lds(kernel_resources, kernel):
    """.group_segment_fixed_size of the kernel: in a kernel's metadata entry the keys are sorted,
    so it is the last such line before the entry's .name."""
    for img in kernel_resources.code_objects(LIB):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(img)
            f.flush()
            notes = subprocess.run([kernel_resources.READELF, "--notes", f.name], capture_output=True,
                                   text=True).stdout
        m = re.search(r"^\s*\.name:\s+\S*%s\S*\s*$" % kernel, notes, flags=re.M)
        if m:
            sizes = re.findall(r"^\s*(?:- )?\.group_segment_fixed_size:\s+(\d+)\s*$", notes[:m.start()], flags=re.M)
            assert int(sizes[-1]) == LDS[kernel], sizes[-1]
            return
    raise AssertionError("kernel not found")
