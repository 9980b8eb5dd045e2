"""CPU: the down-converter bank's entry points (lora_channelize_outputs, lora_channelize_batch)
are declared, exported and bound, count outputs as the header says and refuse bad arguments
before any HIP call (there is no GPU here, so a refusal that needed one would not come back as
LORA_EINVAL); and the host-side helpers of lora_phy_amd.stream around them."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from lora_phy_amd import _capi
from tests import channel_checker as cc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "lora_mi355x.h")
NAMES = {"lora_channelize_outputs": [C.c_int64, C.c_int64, C.c_int64],
         "lora_channelize_batch": [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64,
                                   C.c_int64, C.c_void_p, C.c_int64, C.POINTER(C.c_int32), C.c_int64, C.c_void_p,
                                   C.c_int64, C.c_int, C.c_void_p]}


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


def test_outputs_formula_on_a_grid():
    lib = _capi.lib()
    for T, D in ((65, 8), (7, 3), (3, 8), (1, 1), (512, 64)):
        for L in (0, T - 1, T, T + D - 1, T + D, 10 * T + 3):
            want = 0 if L < T else (L - T) // D + 1
            assert lib.lora_channelize_outputs(L, T, D) == want == cc.outputs(L, T, D), (L, T, D)
    E = _capi.LORA_EINVAL
    assert lib.lora_channelize_outputs(-1, 5, 2) == E and lib.lora_last_error().decode()
    assert lib.lora_channelize_outputs(10, 0, 2) == E
    assert lib.lora_channelize_outputs(10, 5, 0) == E
    assert lib.lora_channelize_outputs(10, -5, 2) == E and lib.lora_channelize_outputs(10, 5, -2) == E


def test_batch_refuses_before_any_hip_call():
    """Every refusal of the header's list, on a machine with no GPU.  The pointers are never
    followed: `steps` is a real host array, the rest are made-up non-NULL addresses."""
    lib = _capi.lib()
    E = _capi.LORA_EINVAL
    steps = (C.c_int32 * 2)(1, -1)
    P = C.c_void_p(4096)

    def call(iq=P, rows=1, row_len=1000, row_stride=1000, first=0, taps=P, ntaps=65, decim=8, nco=P, period=5,
             st=steps, channels=2, out=P, out_stride=200):
        return lib.lora_channelize_batch(iq, rows, row_len, row_stride, first, taps, ntaps, decim, nco, period, st,
                                         channels, out, out_stride, 0, None)

    def refused(**kw):
        rc = call(**kw)
        return rc == E and bool(lib.lora_last_error().decode())

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
    assert refused(out_stride=cc.outputs(1000, 65, 8) - 1)
    assert refused(rows=1 << 40, row_stride=1000)             # a grid beyond 2^31
    # nothing to do is not an error, needs no iq and makes no HIP call: W comes back
    assert call(iq=None, rows=0) == cc.outputs(1000, 65, 8)
    assert call(iq=None, row_len=64, row_stride=64) == 0
    assert call(iq=None, row_len=0, row_stride=0, out_stride=0) == 0


def test_lowpass_taps():
    from lora_phy_amd import stream

    for T, cutoff in ((65, 0.1), (65, 0.2), (33, 0.3), (33, 0.1), (1, 0.5), (512, 0.01)):
        h = stream.lowpass_taps(T, cutoff)
        assert h.dtype == np.float32 and h.shape == (T,)
        assert np.array_equal(h, h[::-1])
        assert abs(float(h.astype(np.float64).sum()) - 1.0) < 1e-6
        j = np.arange(T, dtype=np.float64)
        want = 2 * cutoff * np.sinc(2 * cutoff * (j - (T - 1) / 2)) * np.hamming(T)
        assert np.abs(h - want / want.sum()).max() < 1e-7
    for bad in ((0, 0.1), (65, 0.0), (65, 0.51), (65, -0.1)):
        with pytest.raises(ValueError):
            stream.lowpass_taps(*bad)


def test_the_oscillator_table_is_the_checkers():
    from lora_phy_amd import stream

    for period in (1, 3, 4, 5, 16, 4093, 4096):
        w = stream.nco_table(period)
        wr, wi = cc.nco_table(period)
        assert w.dtype == np.complex64
        assert np.array_equal(w.real.view(np.uint32), wr.view(np.uint32))
        assert np.array_equal(w.imag.view(np.uint32), wi.view(np.uint32))


def test_stream_exports_and_has_no_cpu_fallback():
    import torch

    import lora_phy_amd as amd
    from lora_phy_amd import stream

    assert "Channelizer" in stream.__all__ and "receive_wideband" in stream.__all__ and "lowpass_taps" in stream.__all__
    assert hasattr(amd.LoRaDemod, "work_wideband")
    with pytest.raises(TypeError):
        stream.Channelizer(8, stream.lowpass_taps(65, 0.1), 5, [0, 1], device="cpu")
    for bad in (dict(decim=0), dict(decim=65), dict(period=0), dict(period=4097), dict(steps=[]),
                dict(steps=list(range(33))), dict(taps=np.zeros(513)), dict(taps=np.zeros(0))):
        kw = dict(decim=8, taps=stream.lowpass_taps(65, 0.1), period=5, steps=[0, 1])
        kw.update(bad)
        with pytest.raises(ValueError):
            stream.Channelizer(**kw)
    chan = object.__new__(stream.Channelizer)  # no GPU is needed to reach the argument check
    chan.device, chan.ntaps, chan.decim, chan.channels = torch.device("cuda", 0), 65, 8, 2
    with pytest.raises(TypeError):
        stream.Channelizer.run(chan, torch.zeros(256, dtype=torch.complex64))
