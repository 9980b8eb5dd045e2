"""CPU: the rational-rate bank's entry points (lora_resample_outputs,
lora_resample_channelize_batch) are declared, exported and bound, count outputs as the header
says and refuse bad arguments before any HIP call (there is no GPU here, so a refusal that needed
one would not come back as LORA_EINVAL); and ``stream.Channelizer``'s interp argument."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from lora_phy_amd import _capi
from tests import resample_checker as rc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "lora_mi355x.h")
NAMES = {"lora_resample_outputs": [C.c_int64, C.c_int64, C.c_int64, C.c_int64],
         "lora_resample_channelize_batch": [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p,
                                            C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64,
                                            C.POINTER(C.c_int32), C.c_int64, C.c_void_p, C.c_int64, C.c_int,
                                            C.c_void_p]}


@pytest.mark.parametrize("name", sorted(NAMES))
def test_header_declares_library_exports_and_binding_is_set(name):
    text = open(HEADER).read()
    bare = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert name in re.findall(r"^[A-Za-z_][\w\s\*]*?\b(lora_\w+)\s*\(", bare, flags=re.M)
    assert name in _capi.EXPORTED_SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert name in {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    fn = getattr(_capi.lib(), name)
    assert fn.restype is C.c_int64
    assert list(fn.argtypes) == NAMES[name]
    # the header says whose definition this is
    i = text.index(name + "(")
    assert "the reference has no channelizer" in " ".join(text[text.rindex("/*", 0, i):i].lower().split())


def test_the_batch_entry_is_the_integer_one_with_interp_before_decim():
    """The declared parameter names: lora_channelize_batch's, interp inserted before decim."""
    bare = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)

    def params(name):
        body = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, bare, flags=re.S).group(1)
        return [re.sub(r"[\s\*]+", " ", p).strip() for p in body.split(",")]

    old, new = params("lora_channelize_batch"), params("lora_resample_channelize_batch")
    i = old.index("int64_t decim")
    assert new == old[:i] + ["int64_t interp"] + old[i:]


def test_outputs_formula_on_a_grid():
    lib = _capi.lib()
    for T in (1, 2, 3, 5, 7, 41, 385):
        for Li in (1, 2, 3, 5, 16):
            for D in (1, 3, 5, 8, 96):
                for L in (0, 1, 2, 3, T // Li, T // Li + 1, T // Li + 2, (T + D) // Li + 1, (T + D) // Li + 2, 10 * T + 3):
                    span = (L - 1) * Li + 1
                    want = 0 if L < 1 or span < T else (span - T) // D + 1
                    assert lib.lora_resample_outputs(L, T, Li, D) == want == rc.outputs(L, T, Li, D), (L, T, Li, D)
    # the header's span needs 64 bits: (2^31 - 2) * 16 + 1
    assert lib.lora_resample_outputs((1 << 31) - 1, 4096, 16, 256) == ((((1 << 31) - 2) * 16 + 1) - 4096) // 256 + 1
    E = _capi.LORA_EINVAL
    assert lib.lora_resample_outputs(-1, 5, 2, 3) == E and lib.lora_last_error().decode()
    assert lib.lora_resample_outputs(10, 0, 2, 3) == E
    assert lib.lora_resample_outputs(10, 5, 0, 3) == E
    assert lib.lora_resample_outputs(10, 5, 2, 0) == E
    assert lib.lora_resample_outputs(10, -5, 2, 3) == E and lib.lora_resample_outputs(10, 5, -2, 3) == E
    assert lib.lora_resample_outputs(10, 5, 2, -3) == E
    assert lib.lora_resample_outputs(1 << 62, 5, 4, 8) == E  # row_len * interp beyond 64 bits


def test_batch_refuses_before_any_hip_call():
    """Every refusal of the header's list, on a machine with no GPU.  The pointers are never
    followed: `steps` is a real host array, the rest are made-up non-NULL addresses."""
    lib = _capi.lib()
    E = _capi.LORA_EINVAL
    steps = (C.c_int32 * 2)(1, -1)
    P = C.c_void_p(4096)
    W0 = rc.outputs(1000, 49, 3, 8)

    def call(iq=P, rows=1, row_len=1000, row_stride=1000, first=0, taps=P, ntaps=49, interp=3, decim=8, nco=P,
             period=5, st=steps, channels=2, out=P, out_stride=400):
        return lib.lora_resample_channelize_batch(iq, rows, row_len, row_stride, first, taps, ntaps, interp, decim,
                                                  nco, period, st, channels, out, out_stride, 0, None)

    def refused(**kw):
        rc_ = call(**kw)
        return rc_ == E and bool(lib.lora_last_error().decode())

    assert W0 == 369 and W0 <= 400
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
    # the limits themselves are accepted; nothing to do is not an error, needs no iq and makes no
    # HIP call: W comes back
    assert call(iq=None, rows=0) == W0
    assert call(iq=None, rows=0, out_stride=W0) == W0
    assert call(iq=None, rows=0, ntaps=3 * 512) == rc.outputs(1000, 1536, 3, 8)
    assert call(iq=None, rows=0, ntaps=4096, interp=16, decim=256) == rc.outputs(1000, 4096, 16, 256) == 47
    assert call(iq=None, rows=0, interp=8, decim=8, out_stride=1000) == rc.outputs(1000, 49, 8, 8)
    assert call(iq=None, rows=0, interp=1, ntaps=512, decim=256) == rc.outputs(1000, 512, 1, 256)
    assert call(iq=None, row_len=16, row_stride=16) == 0      # span 46 < 49
    assert call(iq=None, row_len=0, row_stride=0, out_stride=0) == 0


def test_channelizer_checks_interp():
    from lora_phy_amd import stream

    kw = dict(decim=8, taps=stream.lowpass_taps(49, 0.0625, gain=3), period=5, steps=[0, 1])
    for bad in (dict(interp=0), dict(interp=17, decim=32), dict(interp=9), dict(interp=-1),
                dict(interp=3, decim=257), dict(interp=2, taps=np.zeros(1025)), dict(interp=16, decim=16,
                                                                                     taps=np.zeros(4097)),
                dict(interp=1, decim=65), dict(interp=1, taps=np.zeros(513))):
        with pytest.raises(ValueError):
            stream.Channelizer(**{**kw, **bad})
    # the device is looked at after the arguments: a legal rational bank gets as far as that
    with pytest.raises(TypeError):
        stream.Channelizer(**{**kw, "interp": 3, "decim": 256, "taps": np.zeros(1536)}, device="cpu")
    chan = object.__new__(stream.Channelizer)  # no GPU is needed for the host arithmetic
    chan.ntaps, chan.decim, chan.interp, chan._lib = 49, 8, 3, _capi.lib()
    assert chan.delay == 8.0
    for L in (0, 1, 16, 17, 18, 19, 20, 1000):
        assert chan.outputs(L) == chan._outputs(L) == rc.outputs(L, 49, 3, 8)
    chan.interp = 1
    assert chan.delay == 24.0 and chan.outputs(1000) == chan._outputs(1000) == (1000 - 49) // 8 + 1
