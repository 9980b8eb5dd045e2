"""CPU: the propagation stage's entry point (lora_propagate_batch) is declared, exported and bound,
and refuses bad arguments before any HIP call (there is no GPU here, so a refusal that needed one
would not come back as LORA_EINVAL), each rule with a text of its own and in the header's order;
and the host-side word helpers and checks of lora_phy_amd.stream around it."""
import ctypes as C
import os
import re
import subprocess

import pytest

from lora_phy_amd import _capi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "lora_mi355x.h")
NAME = "lora_propagate_batch"
ARGTYPES = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p,
            C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
            C.c_int, C.c_void_p]

# the rules in the header's order: the text of each
T_NEG = "negative rows / in_len / in_stride / in_first / row_len / first_sample / out_stride"
T_LEN = "row_len must be < 2^31"
T_END = "first_sample + row_len must be <= 2^40 and in_first <= 2^41"
T_IN_STRIDE = "in_stride smaller than in_len"
T_OUT_STRIDE = "out_stride smaller than row_len"
T_IN_ALIGN = "in is not aligned to one sample"
T_OUT_ALIGN = "out is not aligned to one sample"
T_OVERLAP = "in and out overlap"
T_PATHS = "paths must be in 1..8"
T_TAPS = "taps must be even and in 2..32"
T_NULL = "null in / delay / gain / table / out"
T_GRID = "batch too large"
A = 1 << 16  # a made-up non-NULL address: `in` and the arrays
ORDER = [T_NEG, T_LEN, T_END, T_IN_STRIDE, T_OUT_STRIDE, T_IN_ALIGN, T_OUT_ALIGN, T_OVERLAP, T_PATHS, T_TAPS, T_NULL,
         T_GRID]


def test_header_declares_library_exports_and_binding_is_set():
    text = open(HEADER).read()
    bare = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert NAME in re.findall(r"^[A-Za-z_][\w\s\*]*?\b(lora_\w+)\s*\(", bare, flags=re.M)
    assert NAME in _capi.EXPORTED_SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert NAME in {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    fn = getattr(_capi.lib(), NAME)
    assert fn.restype is C.c_int64
    assert list(fn.argtypes) == ARGTYPES
    # the header says whose definition this is, whose contract the device-side ranges are, and
    # what is out of scope
    i = text.index(NAME + "(")
    comment = " ".join(w for w in text[text.rindex("/*", 0, i):i].lower().split() if w != "*")
    for word in ("is the library's own", "the caller's contract", "time-varying path gains", "dc offset",
                 "iq imbalance", "must not overlap"):
        assert word in comment, word


def caller():
    """The entry as a function of keyword overrides.  No pointer is ever followed: they are made-up
    non-NULL addresses."""
    lib = _capi.lib()
    P = A
    base = dict(inp=P, rows=2, in_len=1000, in_stride=1000, in_first=0, row_len=900, first=0, paths=2, delay=P,
                gain=P, sfo=P, table=P, taps=16, fcw=P, rate=P, phase=P, out=1 << 20, out_stride=900)

    def call(**kw):
        a = dict(base)
        a.update(kw)
        p = lambda v: None if v is None else C.c_void_p(v)  # noqa: E731
        rc = lib.lora_propagate_batch(p(a["inp"]), a["rows"], a["in_len"], a["in_stride"], a["in_first"],
                                      a["row_len"], a["first"], a["paths"], p(a["delay"]), p(a["gain"]), p(a["sfo"]),
                                      p(a["table"]), a["taps"], p(a["fcw"]), p(a["rate"]), p(a["phase"]), p(a["out"]),
                                      a["out_stride"], 0, None)
        return int(rc), lib.lora_last_error().decode()

    return call


# one call that breaks each rule alone
BREAK = {
    T_NEG: dict(rows=-1),
    T_LEN: dict(row_len=1 << 31, out_stride=1 << 31),
    T_END: dict(first=(1 << 40) - 899),
    T_IN_STRIDE: dict(in_stride=999),
    T_OUT_STRIDE: dict(out_stride=899),
    T_IN_ALIGN: dict(inp=4100),
    T_OUT_ALIGN: dict(out=(1 << 20) + 4),
    T_OVERLAP: dict(out=A + 8 * 1999),
    T_PATHS: dict(paths=0),
    T_TAPS: dict(taps=15),
    T_NULL: dict(delay=None),
    T_GRID: dict(rows=1 << 40, out=1 << 60),
}


def test_every_refusal_has_its_own_text():
    E = _capi.LORA_EINVAL
    call = caller()
    assert len(set(ORDER)) == len(ORDER) == len(BREAK)
    for text in ORDER:
        assert call(**BREAK[text]) == (E, text), text
    # the variants of a rule
    for kw in (dict(in_len=-1), dict(in_stride=-1), dict(in_first=-1), dict(row_len=-1), dict(first=-1),
               dict(out_stride=-1)):
        assert call(**kw) == (E, T_NEG), kw
    assert call(in_first=(1 << 41) + 1) == (E, T_END)
    for kw in (dict(paths=9), dict(paths=-1)):
        assert call(**kw) == (E, T_PATHS), kw
    for kw in (dict(taps=0), dict(taps=1), dict(taps=34), dict(taps=33), dict(taps=-2)):
        assert call(**kw) == (E, T_TAPS), kw
    for kw in (dict(gain=None), dict(table=None), dict(out=None), dict(inp=None)):
        assert call(**kw) == (E, T_NULL), kw
    # overlap: the first and the last byte of either side
    assert call(out=A - 8 * 1799) == (E, T_OVERLAP)           # out's last sample is in's first
    assert call(out=A + 8, in_stride=5000, out_stride=5000) == (E, T_OVERLAP)  # interleaved rows overlap as spans
    # what a rule lets through goes on to a later rule (no legal call is made: on a machine with a
    # GPU it would launch a kernel on these made-up addresses)
    assert call(first=(1 << 40) - 900, delay=None) == (E, T_NULL)            # ends at 2^40 exactly
    assert call(in_first=1 << 41, delay=None) == (E, T_NULL)
    assert call(rows=1, in_stride=1, out_stride=1, delay=None) == (E, T_NULL)  # one row: no stride rule
    assert call(out=A + 8 * 2000, delay=None) == (E, T_NULL)              # out begins where in ends
    assert call(out=A - 8 * 1800, delay=None) == (E, T_NULL)              # out ends where in begins
    assert call(inp=None, in_len=0, in_stride=0, delay=None) == (E, T_NULL)  # no input is not an overlap
    for taps in (2, 32):
        assert call(taps=taps, delay=None) == (E, T_NULL)
    for paths in (1, 8):
        assert call(paths=paths, delay=None) == (E, T_NULL)
    # the optional arrays are optional
    assert call(sfo=None, fcw=None, rate=None, phase=None, delay=None) == (E, T_NULL)


def test_refusals_come_in_the_headers_order():
    """A call that breaks two rules at once is refused with the earlier rule's text, for every
    pair of rules that can be broken together."""
    E = _capi.LORA_EINVAL
    call = caller()
    pairs = 0
    for i, first in enumerate(ORDER):
        for later in ORDER[i + 1:]:
            kw = dict(BREAK[later])
            kw.update(BREAK[first])
            if any(kw[k] != v for k, v in BREAK[later].items()):
                continue  # the two rules need different values of one argument
            assert call(**kw) == (E, first), (first, later)
            pairs += 1
    assert pairs >= 60


def test_nothing_to_do_makes_no_hip_call():
    """rows == 0 or row_len == 0 is not an error, needs no pointer and makes no HIP call (on this
    machine one would fail): row_len comes back.  The rules in front still hold."""
    call = caller()
    none = dict(inp=None, delay=None, gain=None, sfo=None, table=None, fcw=None, rate=None, phase=None, out=None)
    assert call(rows=0)[0] == 900
    assert call(rows=0, **none)[0] == 900
    assert call(row_len=0, out_stride=0)[0] == 0
    assert call(row_len=0, out_stride=0, **none)[0] == 0
    assert call(rows=0, taps=3) == (_capi.LORA_EINVAL, T_TAPS)


def test_stream_exports_and_word_helpers():
    import torch

    import lora_phy_amd as amd
    from lora_phy_amd import stream

    for name in ("propagate", "fracdelay_table", "delay_word", "sfo_word", "cfo_word64", "drift_word"):
        assert name in stream.__all__ and callable(getattr(stream, name)), name
    assert "propagate" in amd.__all__ and amd.propagate is stream.propagate
    # delay_word: to nearest, ties to even, at most 2^15 samples
    assert stream.delay_word(0.0) == 0 and stream.delay_word(0.25) == 1 << 30 and stream.delay_word(-1.5) == -(3 << 31)
    assert stream.delay_word(1.4 / (1 << 32)) == 1 and stream.delay_word(1.6 / (1 << 32)) == 2
    assert stream.delay_word(0.5 / (1 << 32)) == 0 and stream.delay_word(1.5 / (1 << 32)) == 2
    assert stream.delay_word(-1.6 / (1 << 32)) == -2
    assert stream.delay_word(32768.0) == 1 << 47 and stream.delay_word(-32768.0) == -(1 << 47)
    for bad in (32768.001, -32769.0):
        with pytest.raises(ValueError):
            stream.delay_word(bad)
    # sfo_word: 2^-32 sample per sample, at most 2^20
    assert stream.sfo_word(0.0) == 0 and stream.sfo_word(20.0) == 85899 and stream.sfo_word(-40.0) == -171799
    assert stream.sfo_word(244.0) == 1047972
    for bad in (245.0, -300.0):
        with pytest.raises(ValueError):
            stream.sfo_word(bad)
    # cfo_word64: wrapped into int64, and impair's word in its upper half
    assert stream.cfo_word64(0.0) == 0 and stream.cfo_word64(0.25) == 1 << 62 and stream.cfo_word64(-0.25) == -(1 << 62)
    assert stream.cfo_word64(0.5) == stream.cfo_word64(-0.5) == -(1 << 63)
    assert stream.cfo_word64(1.25) == 1 << 62 and stream.cfo_word64(2.0 ** -64) == 1
    for c in (0.125, -0.375, 3.0 / (1 << 32)):
        assert stream.cfo_word64(c) == stream.cfo_word(c) << 32
    with pytest.raises(ValueError):
        stream.cfo_word64(float("nan"))
    # drift_word: Hz per second over fs^2, in 2^-64 cycles per sample per sample
    assert stream.drift_word(0.0, 125e3) == 0
    assert stream.drift_word(100.0, 125e3) == int(round(100.0 / (125e3 * 125e3) * 2.0 ** 64)) == 118059162072
    assert stream.drift_word(-100.0, 250e3) == -29514790518
    for bad in ((1.0, 0.0), (1.0, -5.0), (float("inf"), 1e3), (1e6, 1.0)):
        with pytest.raises(ValueError):
            stream.drift_word(*bad)
    # the table's own argument check
    for bad in (0, 3, 34):
        with pytest.raises(ValueError):
            stream.fracdelay_table(bad)
    assert stream.fracdelay_table(4).shape == (256, 4)
    # propagate: there is no CPU fallback
    with pytest.raises(TypeError):
        stream.propagate(torch.zeros(16, dtype=torch.complex64))
