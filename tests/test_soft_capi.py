"""CPU: the soft-decision entry points (lora_demod_soft_bits_batch,
lora_decode_chain_soft_batch) are declared, exported and bound, and refuse bad parameters
before any HIP call (no GPU is needed: every call here returns from its validation).  The
cases of lora_demod_soft_bits_batch that need a plan (llr_stride < total, sf < 6, the ones
lora_demod_metrics_batch shares) and the kernels are in tests/test_gpu_soft.py."""
import ctypes as C
import os
import re
import subprocess

import pytest

from lora_phy_amd import _capi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "lora_mi355x.h")
SOFT = {"lora_demod_soft_bits_batch": 11, "lora_decode_chain_soft_batch": 12}
EINVAL, ERANGE = _capi.LORA_EINVAL, _capi.LORA_ERANGE
P = 0x1000  # a non-NULL pointer value; validation returns before any buffer is touched


def test_header_declares_library_exports_and_bindings_are_set():
    text = open(HEADER).read()
    bare = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"^[A-Za-z_][\w\s\*]*?\b(lora_\w+)\s*\(", bare, flags=re.M))
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for name, nargs in SOFT.items():
        assert name in declared and name in _capi.EXPORTED_SYMBOLS and name in exported, name
        fn = getattr(_capi.lib(), name)
        assert fn.restype is C.c_int64, name
        assert fn.argtypes is not None and len(fn.argtypes) == nargs, name
        # the header comment carries the definition and cites the reference lines it builds on
        i = text.index(name + "(")
        comment = text[text.rindex("/*", 0, i):i]
        assert re.search(r"\.(cpp|hpp):\d+", comment) and "+0.0f" in comment, name


def test_soft_bits_null_plan_is_rejected_with_a_message():
    lib = _capi.lib()
    assert lib.lora_demod_soft_bits_batch(None, None, 0, 0, 0, None, None, None, None, 0, None) == EINVAL
    assert lib.lora_last_error().decode()
    assert lib.lora_demod_soft_bits_batch(None, P, 1, 128, 128, P, P, P, P, 1, None) == EINVAL


def _soft(sf=7, rdd=4, llr=P, frames=1, S=32, sstride=32, n=14, pay=P, pstride=14):
    return _capi.lib().lora_decode_chain_soft_batch(sf, rdd, llr, frames, S, sstride, n, pay, pstride, None, 0, None)


REJECTED = [
    ("null llr", lambda: _soft(llr=None), EINVAL),
    ("null payload", lambda: _soft(pay=None), EINVAL),
    ("sf 5", lambda: _soft(sf=5), EINVAL),
    ("sf 13", lambda: _soft(sf=13), EINVAL),
    ("rdd -1", lambda: _soft(rdd=-1), EINVAL),
    ("rdd 5", lambda: _soft(rdd=5), EINVAL),
    ("nbytes 256", lambda: _soft(S=8 * 86, sstride=8 * 86, n=256, pstride=256), EINVAL),
    ("nbytes -1", lambda: _soft(n=-1), EINVAL),
    ("sym_stride", lambda: _soft(sstride=31), EINVAL),
    ("payload_stride", lambda: _soft(pstride=13), EINVAL),
    ("negative frames", lambda: _soft(frames=-1), EINVAL),
    ("negative sym_count", lambda: _soft(S=-1, sstride=0, n=0, pstride=0), EINVAL),
    # 2 * nbytes over the codewords sym_count yields: 31 symbols at rdd 4 are 3 blocks, 21 codewords
    ("short frame", lambda: _soft(S=31, sstride=31), ERANGE),
    ("short frame, no block", lambda: _soft(S=7, sstride=7, n=1, pstride=1), ERANGE),
]


@pytest.mark.parametrize("what,call,code", REJECTED, ids=[r[0] for r in REJECTED])
def test_soft_decoder_validation_precedes_any_hip_call(what, call, code):
    assert call() == code, what
    assert _capi.lib().lora_last_error().decode(), what


def test_zero_frames_is_a_no_op_returning_nbytes():
    assert _soft(llr=None, pay=None, frames=0) == 14
    assert _soft(llr=None, pay=None, frames=0, n=0, pstride=0) == 0


def test_wrappers_have_no_cpu_fallback():
    import torch

    import lora_phy_amd as amd
    from lora_phy_amd import codec

    with pytest.raises(TypeError):
        codec.decode_chain_soft(torch.zeros((2, 32, 7)), 7, "4/8", 14)
    plan = object.__new__(amd.DemodPlan)  # no GPU is needed to reach the argument check
    plan.device, plan.mode, plan.step, plan.sf = torch.device("cuda", 0), "raw", 128, 7
    with pytest.raises(TypeError):
        amd.DemodPlan.soft_bits(plan, torch.zeros(256, dtype=torch.complex64))
    plan._h = None  # (close() in __del__ finds nothing to destroy)
    assert hasattr(amd.LoRaDemod, "work_payload_soft")
