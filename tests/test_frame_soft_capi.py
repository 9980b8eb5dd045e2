"""CPU: the two entries of the soft path through the self-describing frame
(lora_demod_soft_bits_frame_batch, lora_decode_frame_soft_batch) are declared, exported and bound,
and reject bad parameters before any HIP call (no GPU is needed: every call here returns from
its validation; the plan's rules that need a plan are in tests/test_gpu_frame_soft.py).  The
kernels are checked by tests/test_gpu_frame_soft.py."""
import ctypes as C
import os
import re
import subprocess

import pytest

from lora_phy_amd import _capi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "lora_mi355x.h")

ENTRIES = ("lora_demod_soft_bits_frame_batch", "lora_decode_frame_soft_batch")
EINVAL = _capi.LORA_EINVAL
P = 0x1000  # a non-NULL, 16-byte aligned pointer value; validation returns before any buffer is touched


def test_header_declares_and_library_exports_the_entries():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"^[A-Za-z_][\w\s\*]*?\b(lora_\w+)\s*\(", text, flags=re.M))
    assert set(ENTRIES) <= declared
    assert set(ENTRIES) <= set(_capi.EXPORTED_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert set(ENTRIES) <= exported


def test_header_states_the_definitions():
    text = open(HEADER).read()
    for name in ENTRIES:
        i = text.index(name + "(")
        comment = text[text.rindex("/*", 0, i):i]
        assert re.search(r"\.(cpp|hpp):\d+", comment), name
    soft = text[:text.index("lora_demod_soft_bits_frame_batch(")]
    soft = soft[soft.rindex("/*"):]
    assert "grayToBinary16(((k + 2) >> 2) & (2^(sf-2) - 1))" in soft and "llr[sf-2] = llr[sf-1] = +0.0f" in soft
    dec = text[:text.index("lora_decode_frame_soft_batch(")]
    dec = dec[dec.rindex("/*"):]
    for phrase in ("L0[(c + bit) % (sf-2)][bit] = llr[bit][c]", "hdr_flips > max_flips", "strict '>'",
                   "bit offset sf - 7"):
        assert phrase in dec, phrase


def test_ctypes_signatures_are_set():
    lib = _capi.lib()
    for name, n in (("lora_demod_soft_bits_frame_batch", 13), ("lora_decode_frame_soft_batch", 19)):
        fn = getattr(lib, name)
        assert fn.restype is C.c_int64, name
        assert fn.argtypes is not None and len(fn.argtypes) == n, name


def _bits(plan=None, iq=P, frames=1, frame_len=1280, stride=1280, llr=P, lstride=10, first=2, count=8):
    return _capi.lib().lora_demod_soft_bits_frame_batch(plan, iq, frames, frame_len, stride, None, None, None, llr,
                                                        lstride, first, count, None)


def _decode(sf=7, llr=P, frames=1, S=38, sstride=38, avail=None, status=P, flips=None, max_flips=5, pay=P, n=16,
            pstride=16):
    return _capi.lib().lora_decode_frame_soft_batch(sf, llr, frames, S, sstride, avail, status, None, None, None,
                                                    None, None, flips, max_flips, pay, n, pstride, 0, None)


REJECTED = [
    ("bits null plan", lambda: _bits()),  # (every rule that reads the plan needs one: the GPU tests)
    ("decode sf 6", lambda: _decode(sf=6)),
    ("decode sf 13", lambda: _decode(sf=13)),
    ("decode negative frames", lambda: _decode(frames=-1)),
    ("decode negative sym_count", lambda: _decode(S=-1)),
    ("decode sym_count 2^31", lambda: _decode(S=1 << 31, sstride=1 << 31)),
    ("decode sym_stride", lambda: _decode(sstride=37)),
    ("decode max_flips -1", lambda: _decode(max_flips=-1)),
    ("decode max_flips 41", lambda: _decode(max_flips=41)),
    ("decode max_bytes 256", lambda: _decode(n=256, pstride=256)),
    ("decode max_bytes -1", lambda: _decode(n=-1)),
    ("decode payload_stride", lambda: _decode(pstride=15)),
    ("decode null llr", lambda: _decode(llr=None)),
]


@pytest.mark.parametrize("what,call", REJECTED, ids=[r[0] for r in REJECTED])
def test_validation_precedes_any_hip_call(what, call):
    lib = _capi.lib()
    assert call() == EINVAL, what
    assert lib.lora_last_error().decode(), what


def test_nothing_to_do_is_a_no_op_returning_the_per_frame_count():
    assert _decode(llr=None, pay=None, status=None, frames=0) == 0   # a NULL payload: header-only mode
    assert _decode(llr=None, frames=0) == 16
    assert _decode(llr=None, frames=0, max_flips=0) == 16 and _decode(llr=None, frames=0, max_flips=40) == 16
    assert _decode(pay=None, status=None) == 0                       # no output asked for
    assert _decode(pay=None, status=None, flips=P, max_flips=41) == EINVAL


def test_wrappers_have_no_cpu_fallback_and_check_their_arguments():
    import torch

    from lora_phy_amd import codec, stream

    llr = torch.zeros((2, 24, 7))
    with pytest.raises(TypeError):
        codec.decode_frame_soft(llr, 7)
    with pytest.raises(TypeError):
        codec.decode_header_soft(llr, 7)
    assert codec.MAX_HDR_FLIPS == 40
    fields = codec.FrameResult(*([None] * 7))
    assert fields.hdr_flips is None  # the hard decoders leave it so
    assert "llr" in stream.StreamPackets.__dataclass_fields__
    import inspect

    for fn in (stream.receive_frames_device, stream.receive_wideband_frames_device):
        p = inspect.signature(fn).parameters
        assert p["soft"].default is False and p["max_flips"].default == 5, fn
    from lora_phy_amd import LoRaDemod, awgn
    from lora_phy_amd.demod import DemodPlan

    p = inspect.signature(LoRaDemod.work_packets_device).parameters
    assert p["soft"].default is False and p["max_flips"].default == 5
    assert inspect.signature(awgn.sweep_receive_frames).parameters["soft"].default is False
    assert inspect.signature(DemodPlan.soft_bits).parameters["reduced"].default is None
