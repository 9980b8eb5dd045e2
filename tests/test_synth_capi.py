"""CPU: the synthesis bank's entry points (lora_synthesize_outputs, lora_synthesize_batch,
lora_synthesize_raw_batch) are declared, exported and bound, count outputs as the header says and
refuse bad arguments before any HIP call (there is no GPU here, so a refusal that needed one would
not come back as LORA_EINVAL); and the host-side checks of lora_phy_amd.stream around them."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from lora_phy_amd import _capi
from tests import synth_checker as sy

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "lora_mi355x.h")
FLOAT = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
         C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
NAMES = {"lora_synthesize_outputs": [C.c_int64, C.c_int64, C.c_int64],
         "lora_synthesize_batch": FLOAT,
         "lora_synthesize_raw_batch": FLOAT[:14] + [C.c_int, C.c_float] + FLOAT[14:]}


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
    # the header says whose definition this is, and what is out of scope
    i = text.index(name + "(")
    comment = " ".join(w for w in text[text.rindex("/*", 0, i):i].lower().split() if w != "*")
    assert "the reference has no synthesiser" in comment
    assert "a rational up-rate (interp / decim) is not" in comment


def test_outputs_formula_on_a_grid():
    lib = _capi.lib()
    for T, U in ((65, 8), (7, 3), (3, 8), (1, 1), (512, 64), (512, 1), (8, 8), (9, 8)):
        P = -(-T // U)
        for Lc in (0, P - 1, P, P + 1, 10 * P + 3):
            want = 0 if Lc < P else (Lc - P + 1) * U
            assert lib.lora_synthesize_outputs(Lc, T, U) == want == sy.outputs(Lc, T, U), (Lc, T, U)
    E = _capi.LORA_EINVAL
    assert lib.lora_synthesize_outputs(-1, 5, 2) == E and lib.lora_last_error().decode()
    assert lib.lora_synthesize_outputs(10, 0, 2) == E
    assert lib.lora_synthesize_outputs(10, 5, 0) == E
    assert lib.lora_synthesize_outputs(10, -5, 2) == E and lib.lora_synthesize_outputs(10, 5, -2) == E
    assert lib.lora_synthesize_outputs(1 << 62, 5, 4) == E  # chan_len * interp beyond 64 bits


def callers():
    """(float entry, raw entry) as functions of keyword overrides.  The device pointers are never
    followed: they are made-up non-NULL addresses; `steps` and `gains` are real host arrays."""
    lib = _capi.lib()
    steps = (C.c_int32 * 2)(1, -1)
    gains = (C.c_float * 2)(1.0, 0.5)
    P = C.c_void_p(4096)
    base = dict(inp=P, rows=1, chan_len=100, in_stride=100, first=0, taps=P, ntaps=65, interp=8, nco=P, period=5,
                st=steps, g=gains, channels=2, out=P, out_stride=736, fmt=_capi.LORA_IQ_CS16, inv=32768.0)

    def call(raw, **kw):
        a = dict(base)
        a.update(kw)
        head = (a["inp"], a["rows"], a["chan_len"], a["in_stride"], a["first"], a["taps"], a["ntaps"], a["interp"],
                a["nco"], a["period"], a["st"], a["g"], a["channels"], a["out"])
        if raw:
            return lib.lora_synthesize_raw_batch(*head, a["fmt"], a["inv"], a["out_stride"], 0, None)
        return lib.lora_synthesize_batch(*head, a["out_stride"], 0, None)

    return call


@pytest.mark.parametrize("raw", [False, True])
def test_batch_refuses_before_any_hip_call(raw):
    """Every refusal of the header's list, on a machine with no GPU."""
    lib = _capi.lib()
    E = _capi.LORA_EINVAL
    call = callers()
    W = sy.outputs(100, 65, 8)
    assert W == 736

    def refused(**kw):
        rc = call(raw, **kw)
        return rc == E and bool(lib.lora_last_error().decode())

    # a NULL pointer with work to do
    for name in ("inp", "taps", "nco", "st", "g", "out"):
        assert refused(**{name: None}), name
    assert refused(rows=-1) and refused(chan_len=-1) and refused(in_stride=-1) and refused(out_stride=-1)
    assert refused(first=-1)
    assert refused(interp=0) and refused(interp=65) and refused(interp=-2)
    assert refused(ntaps=0) and refused(ntaps=513) and refused(ntaps=-3)
    assert refused(period=0) and refused(period=4097)
    assert refused(channels=0) and refused(channels=33)
    assert refused(chan_len=1 << 28, in_stride=1 << 28)           # chan_len * interp == 2^31
    assert refused(chan_len=1 << 31, in_stride=1 << 31, interp=1)
    assert refused(in_stride=99)                                  # two streams
    assert refused(rows=2, channels=1, in_stride=99)
    assert refused(rows=2, out_stride=W - 1)
    assert refused(rows=1 << 40, out_stride=W)                    # a grid beyond 2^31
    if raw:
        assert refused(fmt=0) and refused(fmt=4) and refused(fmt=-1)
        assert refused(out=C.c_void_p(4098), fmt=_capi.LORA_IQ_CS16)      # cs16: 4 bytes
        assert refused(out=C.c_void_p(4097), fmt=_capi.LORA_IQ_CS8)       # 8-bit formats: 2 bytes
        assert refused(out=C.c_void_p(4097), fmt=_capi.LORA_IQ_CU8)
    else:
        assert refused(out=C.c_void_p(4100))                              # complex64: 8 bytes


@pytest.mark.parametrize("raw", [False, True])
def test_nothing_to_do_makes_no_hip_call(raw):
    """rows == 0 or W == 0 is not an error, needs no pointer and makes no HIP call (on this
    machine one would fail): W comes back."""
    call = callers()
    W = sy.outputs(100, 65, 8)
    none = dict(inp=None, taps=None, nco=None, st=None, g=None, out=None)
    assert call(raw, rows=0) == W
    assert call(raw, rows=0, **none) == W
    assert call(raw, chan_len=8, in_stride=8) == 0                # P - 1 samples
    assert call(raw, chan_len=8, in_stride=8, **none) == 0
    assert call(raw, chan_len=0, in_stride=0, out_stride=0, **none) == 0


def test_stream_exports_and_has_no_cpu_fallback():
    import torch

    import lora_phy_amd as amd
    from lora_phy_amd import stream

    assert "Synthesizer" in stream.__all__ and "transmit_wideband" in stream.__all__
    assert hasattr(amd.LoRaMod, "work_wideband")
    taps = stream.lowpass_taps(65, 0.5 / 8, gain=8)
    with pytest.raises(TypeError):
        stream.Synthesizer(8, taps, 5, [0, 1], device="cpu")
    for bad in (dict(interp=0), dict(interp=65), dict(period=0), dict(period=4097), dict(steps=[]),
                dict(steps=list(range(33))), dict(taps=np.zeros(513)), dict(taps=np.zeros(0)),
                dict(gains=[1.0]), dict(gains=[1.0, 2.0, 3.0])):
        kw = dict(interp=8, taps=taps, period=5, steps=[0, 1])
        kw.update(bad)
        with pytest.raises(ValueError):
            stream.Synthesizer(**kw)
    syn = object.__new__(stream.Synthesizer)  # no GPU is needed to reach the argument checks
    syn.device, syn.ntaps, syn.interp, syn.channels, syn.P = torch.device("cuda", 0), 65, 8, 2, 9
    assert syn.delay == sy.delay(65, 8) == -32.0
    with pytest.raises(TypeError):
        stream.Synthesizer.run(syn, torch.zeros((2, 256), dtype=torch.complex64))
    with pytest.raises(ValueError):
        stream.Synthesizer.run(syn, torch.zeros((2, 256), dtype=torch.complex64), inv_scale=128.0)
    with pytest.raises(TypeError):
        stream.Synthesizer.run(syn, torch.zeros((2, 256), dtype=torch.complex64), dtype=torch.int32)
    with pytest.raises(TypeError):
        stream.transmit_wideband(syn, torch.zeros((1, 16), dtype=torch.complex64), [0], [0], 64)
