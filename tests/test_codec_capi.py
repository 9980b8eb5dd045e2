"""CPU: the payload codec's C-ABI (lora_decode_batch, lora_encode_batch,
lora_decode_chain_batch, lora_encode_chain_batch, lora_chain_symbols) is declared, exported
and bound, and rejects bad parameters before any HIP call (no GPU is needed: every call
here returns from its validation).  The kernels themselves are checked by
tests/test_gpu_codec.py on the GPU."""
import ctypes as C
import os
import re
import subprocess

import pytest

from lora_phy_amd import _capi, codes

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "lora_mi355x.h")
CODEC = ("lora_decode_batch", "lora_encode_batch", "lora_decode_chain_batch", "lora_encode_chain_batch",
         "lora_chain_symbols")
EINVAL, ERANGE = _capi.LORA_EINVAL, _capi.LORA_ERANGE
P = 0x1000  # a non-NULL pointer value; validation returns before any buffer is touched


def test_header_declares_and_library_exports_the_codec():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"^[A-Za-z_][\w\s\*]*?\b(lora_\w+)\s*\(", text, flags=re.M))
    assert set(CODEC) <= declared
    assert set(CODEC) <= set(_capi.EXPORTED_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert set(CODEC) <= exported


def test_header_cites_the_reference_for_each_function():
    text = open(HEADER).read()
    for name in CODEC:
        i = text.index(name + "(")
        comment = text[text.rindex("/*", 0, i):i]
        assert re.search(r"\.(cpp|hpp):\d+", comment), name


def test_ctypes_signatures_are_set():
    lib = _capi.lib()
    nargs = {"lora_decode_batch": 11, "lora_encode_batch": 9, "lora_decode_chain_batch": 12,
             "lora_encode_chain_batch": 10, "lora_chain_symbols": 3}
    for name, n in nargs.items():
        fn = getattr(lib, name)
        assert fn.restype is C.c_int64, name
        assert fn.argtypes is not None and len(fn.argtypes) == n, name


def _decode(sym=P, frames=1, S=16, sstride=16, pay=P, pstride=8):
    return _capi.lib().lora_decode_batch(sym, frames, S, sstride, pay, pstride, None, None, None, 0, None)


def _encode(pay=P, frames=1, n=8, pstride=8, crc=0, sym=P, sstride=None):
    sstride = 2 * (n + 2 * crc) if sstride is None else sstride
    return _capi.lib().lora_encode_batch(pay, frames, n, pstride, crc, sym, sstride, 0, None)


def _decode_chain(sf=7, rdd=4, sym=P, frames=1, S=32, sstride=32, n=14, pay=P, pstride=14):
    return _capi.lib().lora_decode_chain_batch(sf, rdd, sym, frames, S, sstride, n, pay, pstride, None, 0, None)


def _encode_chain(sf=7, rdd=4, pay=P, frames=1, n=14, pstride=14, sym=P, sstride=32):
    return _capi.lib().lora_encode_chain_batch(sf, rdd, pay, frames, n, pstride, sym, sstride, 0, None)


REJECTED = [
    # a NULL required pointer
    ("decode null symbols", lambda: _decode(sym=None), EINVAL),
    ("decode null payload", lambda: _decode(pay=None), EINVAL),
    ("encode null payload", lambda: _encode(pay=None), EINVAL),
    ("encode null symbols", lambda: _encode(sym=None), EINVAL),
    ("decode_chain null symbols", lambda: _decode_chain(sym=None), EINVAL),
    ("decode_chain null payload", lambda: _decode_chain(pay=None), EINVAL),
    ("encode_chain null payload", lambda: _encode_chain(pay=None), EINVAL),
    ("encode_chain null symbols", lambda: _encode_chain(sym=None), EINVAL),
    # sf outside 6..12, rdd outside 0..4, nbytes over 255
    ("decode_chain sf 5", lambda: _decode_chain(sf=5), EINVAL),
    ("decode_chain sf 13", lambda: _decode_chain(sf=13), EINVAL),
    ("decode_chain rdd -1", lambda: _decode_chain(rdd=-1), EINVAL),
    ("decode_chain rdd 5", lambda: _decode_chain(rdd=5), EINVAL),
    ("decode_chain nbytes 256", lambda: _decode_chain(S=8 * 86, sstride=8 * 86, n=256, pstride=256), EINVAL),
    ("encode_chain sf 5", lambda: _encode_chain(sf=5), EINVAL),
    ("encode_chain sf 13", lambda: _encode_chain(sf=13), EINVAL),
    ("encode_chain rdd -1", lambda: _encode_chain(rdd=-1), EINVAL),
    ("encode_chain rdd 5", lambda: _encode_chain(rdd=5), EINVAL),
    ("encode_chain nbytes 256", lambda: _encode_chain(n=256, pstride=256, sstride=4096), EINVAL),
    ("encode nbytes 256", lambda: _encode(n=256, pstride=256), EINVAL),
    ("chain_symbols sf 5", lambda: _capi.lib().lora_chain_symbols(5, 1, 4), EINVAL),
    ("chain_symbols sf 13", lambda: _capi.lib().lora_chain_symbols(13, 1, 4), EINVAL),
    ("chain_symbols rdd 5", lambda: _capi.lib().lora_chain_symbols(7, 5, 4), EINVAL),
    ("chain_symbols nbytes 256", lambda: _capi.lib().lora_chain_symbols(7, 1, 256), EINVAL),
    # a stride smaller than the row
    ("decode sym_stride", lambda: _decode(sstride=15), EINVAL),
    ("decode payload_stride", lambda: _decode(pstride=7), EINVAL),
    ("encode payload_stride", lambda: _encode(pstride=7), EINVAL),
    ("encode sym_stride", lambda: _encode(sstride=15), EINVAL),
    ("encode sym_stride with crc", lambda: _encode(crc=1, sstride=16), EINVAL),
    ("decode_chain sym_stride", lambda: _decode_chain(sstride=31), EINVAL),
    ("decode_chain payload_stride", lambda: _decode_chain(pstride=13), EINVAL),
    ("encode_chain payload_stride", lambda: _encode_chain(pstride=13), EINVAL),
    ("encode_chain sym_stride", lambda: _encode_chain(sstride=31), EINVAL),
    # negative sizes
    ("decode negative frames", lambda: _decode(frames=-1), EINVAL),
    ("encode negative nbytes", lambda: _encode(n=-1), EINVAL),
    # 2 * nbytes over the codewords sym_count yields: 31 symbols at rdd 4 are 3 blocks, 21 codewords
    ("decode_chain short frame", lambda: _decode_chain(S=31, sstride=31), ERANGE),
    ("decode_chain short frame, no block", lambda: _decode_chain(S=7, sstride=7, n=1, pstride=1), ERANGE),
]


@pytest.mark.parametrize("what,call,code", REJECTED, ids=[r[0] for r in REJECTED])
def test_validation_precedes_any_hip_call(what, call, code):
    lib = _capi.lib()
    assert call() == code, what
    assert lib.lora_last_error().decode(), what
    with pytest.raises(_capi.LoraError):
        _capi.check(code)


def test_zero_frames_is_a_no_op_returning_the_per_frame_count():
    assert _decode(sym=None, pay=None, frames=0, S=17, sstride=17) == 8
    assert _encode(pay=None, sym=None, frames=0) == 16
    assert _encode(pay=None, sym=None, frames=0, crc=1) == 20
    assert _decode_chain(sym=None, pay=None, frames=0) == 14
    assert _encode_chain(pay=None, sym=None, frames=0) == 32


@pytest.mark.parametrize("sf", range(6, 13))
def test_chain_symbols_equals_the_host_chain(sf):
    lib = _capi.lib()
    for rdd in range(5):
        for n in (0, 1, 3, 255):
            assert lib.lora_chain_symbols(sf, rdd, n) == len(codes.encode_chain(bytes(n), sf, rdd)["symbols"]), \
                (sf, rdd, n)


def test_wrappers_have_no_cpu_fallback():
    import torch

    from lora_phy_amd import codec

    pay = torch.zeros((2, 8), dtype=torch.uint8)
    sym = torch.zeros((2, 16), dtype=torch.uint16)
    with pytest.raises(TypeError):
        codec.encode(pay)
    with pytest.raises(TypeError):
        codec.encode(pay, append_crc=True)
    with pytest.raises(TypeError):
        codec.decode(sym)
    with pytest.raises(TypeError):
        codec.encode_chain(pay, 7, "4/8")
    with pytest.raises(TypeError):
        codec.decode_chain(sym, 7, "4/8", 7)


def test_codec_is_exported():
    import lora_phy_amd

    assert lora_phy_amd.codec.decode and "codec" in lora_phy_amd.__all__
    assert hasattr(lora_phy_amd.LoRaDemod, "work_payload") and hasattr(lora_phy_amd.LoRaMod, "work_payload")
