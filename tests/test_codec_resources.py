"""CPU: the payload codec's kernels (csrc/lora_codec.hip) keep no scratch - code-object
metadata of the built library, read as tests/test_kernel_resources.py reads it."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "lora-sdr-lightweight-standalone-library-_amd", "lora_phy_amd", "lib", "liblora_mi355x.so")
CODEC_KERNELS = ("k_codec_decode", "k_codec_encode", "k_codec_chain_decode", "k_codec_chain_encode")


@pytest.fixture(scope="module")
def codec_kernels():
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    import kernel_resources

    if not os.path.exists(kernel_resources.READELF):
        pytest.skip("llvm-readelf not available")
    out = {}
    for r in kernel_resources.kernels(LIB):
        m = re.search(r"\b(k_codec_\w+)", r.get("demangled", r["name"]))
        if m:
            out.setdefault(m.group(1), r)
    return out


def test_every_codec_kernel_is_in_the_library(codec_kernels):
    assert sorted(codec_kernels) == sorted(CODEC_KERNELS)


@pytest.mark.parametrize("name", CODEC_KERNELS)
def test_codec_kernel_has_no_scratch(codec_kernels, name):
    r = codec_kernels[name]
    assert r.get("private_segment_fixed_size", 0) == 0, (name, r)
    assert r.get("vgpr_spill_count", 0) == 0, (name, r)
    assert r.get("sgpr_spill_count", 0) == 0, (name, r)
