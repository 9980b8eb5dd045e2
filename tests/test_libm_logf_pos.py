"""CPU: lm_logf_pos_k (csrc/lora_libm.h), the branch-free lockstep logf of the impairment kernel's
Box-Muller step, equals this host's glibc bit for bit on every value the kernel can ask for - all
2^23 of u = (2 m + 1) * 2^-24 - and on a strided sweep of the positive normal floats.  Builds
tests/native/logf_pos_check.cpp with g++, as tests/test_libm_host.py builds its program."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "logf_pos_check.cpp")
BIN = os.path.join(HERE, "native", "logf_pos_check")
HDR = os.path.join(HERE, "..", "lora-sdr-lightweight-standalone-library-_amd", "csrc", "lora_libm.h")


@pytest.fixture(scope="module")
def results():
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-o", BIN, SRC, "-lm"])
    out = subprocess.run([BIN], capture_output=True, text=True, check=True, timeout=300).stdout
    return {name: (int(n), int(bad)) for name, n, bad in (line.split() for line in out.splitlines())}


@pytest.mark.parametrize("name,least", [("box_muller_u", 1 << 23), ("positive_normals", 30_000_000)])
def test_bit_exact_vs_glibc(results, name, least):
    n, bad = results[name]
    assert n >= least
    assert bad == 0, f"{name}: {bad} of {n} differ from glibc"
