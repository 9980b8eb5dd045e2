"""CPU: the banks' raw entries (lora_channelize_raw_batch, lora_resample_channelize_raw_batch) are
declared, exported and bound, and refuse bad arguments before any HIP call - their own rules
(format, alignment of iq to one sample) and every rule of their float counterparts, restated
from tests/test_channel_capi.py and tests/test_resample_capi.py (there is no GPU here, so a
refusal that needed one would not come back as LORA_EINVAL)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from lora_phy_amd import _capi
from tests import channel_checker as cc
from tests import resample_checker as rc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "lora_mi355x.h")
RAW = [C.c_void_p, C.c_int, C.c_float]
NAMES = {"lora_channelize_raw_batch": "lora_channelize_batch",
         "lora_resample_channelize_raw_batch": "lora_resample_channelize_batch"}
FORMATS = {"cs16": (_capi.LORA_IQ_CS16, 4), "cs8": (_capi.LORA_IQ_CS8, 2), "cu8": (_capi.LORA_IQ_CU8, 2)}


def test_format_constants():
    text = open(HEADER).read()
    for name, value in (("LORA_IQ_CS16", 1), ("LORA_IQ_CS8", 2), ("LORA_IQ_CU8", 3)):
        assert re.search(r"^#define %s %d\b" % (name, value), text, flags=re.M)
        assert getattr(_capi, name) == value


@pytest.mark.parametrize("name", sorted(NAMES))
def test_header_declares_library_exports_and_binding_is_set(name):
    text = open(HEADER).read()
    bare = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert name in re.findall(r"^[A-Za-z_][\w\s\*]*?\b(lora_\w+)\s*\(", bare, flags=re.M)
    assert name in _capi.EXPORTED_SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert name in {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    fn, flt = getattr(_capi.lib(), name), getattr(_capi.lib(), NAMES[name])
    assert fn.restype is C.c_int64
    # the float counterpart argument for argument, with (iq, format, scale) in place of iq
    assert list(fn.argtypes) == RAW + list(flt.argtypes)[1:]
    i = text.index(name + "(")
    assert "the reference has no channelizer" in " ".join(text[text.rindex("/*", 0, i):i].lower().split())


def refusals(call, lib):
    E = _capi.LORA_EINVAL

    def refused(**kw):
        got = call(**kw)
        return got == E and bool(lib.lora_last_error().decode())

    return refused


@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_integer_bank_refuses_before_any_hip_call(fmt):
    """The pointers are never followed: `steps` is a real host array, the rest are made-up non-NULL
    addresses."""
    lib = _capi.lib()
    format_, size = FORMATS[fmt]
    steps = (C.c_int32 * 2)(1, -1)
    P = C.c_void_p(4096)

    def call(iq=P, format=format_, scale=1.0, rows=1, row_len=1000, row_stride=1000, first=0, taps=P, ntaps=65,
             decim=8, nco=P, period=5, st=steps, channels=2, out=P, out_stride=200):
        return lib.lora_channelize_raw_batch(iq, format, scale, rows, row_len, row_stride, first, taps, ntaps, decim,
                                             nco, period, st, channels, out, out_stride, 0, None)

    refused = refusals(call, lib)
    W0 = cc.outputs(1000, 65, 8)
    # the raw entries' own rules
    assert refused(format=0) and refused(format=4) and refused(format=-1)
    assert refused(format=0, rows=0) and refused(format=4, iq=None, rows=0)   # even with nothing to do
    for k in range(1, size):
        assert refused(iq=C.c_void_p(4096 + k)) and refused(iq=C.c_void_p(4096 + k), rows=0)
    # one sample is all the alignment asked for: an iq off the 16-byte grid is accepted
    for k in range(1, 16 // size):
        assert call(iq=C.c_void_p(4096 + k * size), rows=0) == W0
    # the float entry's rules
    assert refused(taps=None) and refused(nco=None) and refused(st=None) and refused(out=None)
    assert refused(iq=None)                                   # work to do
    assert refused(rows=-1) and refused(row_len=-1) and refused(row_stride=-1) and refused(out_stride=-1)
    assert refused(first=-1)
    assert refused(ntaps=0) and refused(ntaps=513) and refused(ntaps=-3)
    assert refused(decim=0) and refused(decim=65)
    assert refused(period=0) and refused(period=4097)
    assert refused(channels=0) and refused(channels=33)
    assert refused(row_len=1 << 31, row_stride=1 << 31)
    assert refused(rows=2, row_stride=999)
    assert refused(out_stride=W0 - 1)
    assert refused(rows=1 << 40, row_stride=1000)             # a grid beyond 2^31
    # nothing to do is not an error, needs no iq and makes no HIP call: W comes back; and the
    # scale is not checked
    assert call(iq=None, rows=0) == W0
    assert call(iq=None, rows=0, scale=float("nan")) == W0 and call(iq=None, rows=0, scale=float("inf")) == W0
    assert call(iq=None, row_len=64, row_stride=64) == 0
    assert call(iq=None, row_len=0, row_stride=0, out_stride=0) == 0


@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_rational_bank_refuses_before_any_hip_call(fmt):
    lib = _capi.lib()
    format_, size = FORMATS[fmt]
    steps = (C.c_int32 * 2)(1, -1)
    P = C.c_void_p(4096)
    W0 = rc.outputs(1000, 49, 3, 8)

    def call(iq=P, format=format_, scale=1.0, rows=1, row_len=1000, row_stride=1000, first=0, taps=P, ntaps=49,
             interp=3, decim=8, nco=P, period=5, st=steps, channels=2, out=P, out_stride=400):
        return lib.lora_resample_channelize_raw_batch(iq, format, scale, rows, row_len, row_stride, first, taps,
                                                      ntaps, interp, decim, nco, period, st, channels, out,
                                                      out_stride, 0, None)

    refused = refusals(call, lib)
    assert W0 == 369 and W0 <= 400
    # the raw entries' own rules
    assert refused(format=0) and refused(format=4) and refused(format=-1)
    assert refused(format=0, rows=0) and refused(format=4, iq=None, rows=0)
    for k in range(1, size):
        assert refused(iq=C.c_void_p(4096 + k)) and refused(iq=C.c_void_p(4096 + k), rows=0)
    for k in range(1, 16 // size):
        assert call(iq=C.c_void_p(4096 + k * size), rows=0) == W0
    # the float entry's rules
    assert refused(taps=None) and refused(nco=None) and refused(st=None) and refused(out=None)
    assert refused(iq=None)                                   # work to do
    assert refused(rows=-1) and refused(row_len=-1) and refused(row_stride=-1) and refused(out_stride=-1)
    assert refused(first=-1)
    assert refused(interp=0) and refused(interp=17, decim=32) and refused(interp=-2)
    assert refused(decim=0) and refused(decim=257) and refused(decim=-8)
    assert refused(interp=9, decim=8) and refused(interp=2, decim=1)   # a rate-reducing bank only
    assert refused(ntaps=0) and refused(ntaps=4097, interp=16, decim=16) and refused(ntaps=-3)
    assert refused(ntaps=3 * 512 + 1) and refused(ntaps=513, interp=1)  # more than 512 taps per phase
    assert refused(period=0) and refused(period=4097)
    assert refused(channels=0) and refused(channels=33)
    assert refused(row_len=1 << 31, row_stride=1 << 31, out_stride=1 << 31)
    assert refused(rows=2, row_stride=999)
    assert refused(out_stride=W0 - 1)
    assert refused(rows=1 << 40, row_stride=1000)             # a grid beyond 2^31
    assert call(iq=None, rows=0) == W0
    assert call(iq=None, rows=0, ntaps=4096, interp=16, decim=256) == rc.outputs(1000, 4096, 16, 256) == 47
    assert call(iq=None, row_len=16, row_stride=16) == 0      # span 46 < 49
