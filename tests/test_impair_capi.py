"""CPU: the channel impairment stage's entry points (lora_impair_batch, lora_impair_raw_batch) are
declared, exported and bound, and refuse bad arguments before any HIP call (there is no GPU here,
so a refusal that needed one would not come back as LORA_EINVAL), each rule with a text of its
own and in the header's order; and the host-side checks of lora_phy_amd.stream around them."""
import ctypes as C
import math
import os
import re
import subprocess

import pytest

from lora_phy_amd import _capi
from tests import impair_checker as ic

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "lora_mi355x.h")
FLOAT = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_uint64, C.c_void_p, C.c_void_p,
         C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
NAMES = {"lora_impair_batch": FLOAT, "lora_impair_raw_batch": FLOAT[:12] + [C.c_int, C.c_float] + FLOAT[12:]}

# the rules in the header's order: the text of each
T_NEG = "negative rows / row_len / in_stride / out_stride / first_sample / first_row"
T_LEN = "row_len must be < 2^31"
T_IN_STRIDE = "in_stride smaller than row_len"
T_OUT_STRIDE = "out_stride smaller than row_len"
T_INPLACE = "out == in needs in_stride == out_stride"
T_IN_ALIGN = "in is not aligned to one sample"
T_OUT_ALIGN = "out is not aligned to one sample"
T_FORMAT = "format must be LORA_IQ_CS16, LORA_IQ_CS8 or LORA_IQ_CU8"
T_GRID = "batch too large"
T_OUT = "null out"
T_SIGMA = "noise-only rows (in == NULL) need sigma"
T_NOTHING = "nothing to do: gain, fcw, phase and sigma are all NULL"
ORDER = [T_NEG, T_LEN, T_IN_STRIDE, T_OUT_STRIDE, T_INPLACE, T_IN_ALIGN, T_OUT_ALIGN, T_FORMAT, T_GRID, T_OUT,
         T_SIGMA, T_NOTHING]


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
    assert "is the library's own" in comment
    for word in ("fractional delay", "multipath", "frequency drift", "dc offset", "iq imbalance",
                 "an integer delay is the caller's slice"):
        assert word in comment, word


def caller():
    """The entries as a function of keyword overrides.  No pointer is ever followed: they are
    made-up non-NULL addresses."""
    lib = _capi.lib()
    P = 4096
    base = dict(inp=P, rows=2, row_len=1000, in_stride=1000, first=0, first_row=0, seed=1, gain=P, fcw=P, phase=P,
                sigma=P, out=8192, out_stride=1000, fmt=_capi.LORA_IQ_CS16, inv=32768.0)

    def call(raw, **kw):
        a = dict(base)
        a.update(kw)
        p = lambda v: None if v is None else C.c_void_p(v)  # noqa: E731
        head = (p(a["inp"]), a["rows"], a["row_len"], a["in_stride"], a["first"], a["first_row"], a["seed"],
                p(a["gain"]), p(a["fcw"]), p(a["phase"]), p(a["sigma"]), p(a["out"]))
        if raw:
            rc = lib.lora_impair_raw_batch(*head, a["fmt"], a["inv"], a["out_stride"], 0, None)
        else:
            rc = lib.lora_impair_batch(*head, a["out_stride"], 0, None)
        return int(rc), lib.lora_last_error().decode()

    return call


# one call that breaks each rule alone (raw: None = both entries)
ALL_NULL = dict(gain=None, fcw=None, phase=None, sigma=None)
BREAK = {
    T_NEG: dict(rows=-1),
    T_LEN: dict(row_len=1 << 31, in_stride=1 << 31, out_stride=1 << 31),
    T_IN_STRIDE: dict(in_stride=999),
    T_OUT_STRIDE: dict(out_stride=999),
    T_INPLACE: dict(out=4096, out_stride=1001),
    T_IN_ALIGN: dict(inp=4100),
    T_OUT_ALIGN: dict(out=8193),
    T_FORMAT: dict(fmt=0),
    T_GRID: dict(rows=1 << 40),
    T_OUT: dict(out=None),
    T_SIGMA: dict(inp=None, sigma=None),
    T_NOTHING: dict(ALL_NULL),
}


@pytest.mark.parametrize("raw", [False, True])
def test_every_refusal_has_its_own_text(raw):
    E = _capi.LORA_EINVAL
    call = caller()
    assert len(set(ORDER)) == len(ORDER) == len(BREAK)
    for text in ORDER:
        if text == T_FORMAT and not raw:
            continue
        assert call(raw, **BREAK[text]) == (E, text), text
    # the variants of a rule
    for kw in (dict(row_len=-1), dict(in_stride=-1), dict(out_stride=-1), dict(first=-1), dict(first_row=-1)):
        assert call(raw, **kw) == (E, T_NEG), kw
    # what a rule lets through goes on to a later rule (no legal call is made: on a machine with
    # a GPU it would launch a kernel on these made-up addresses)
    assert call(raw, rows=1, in_stride=999, out_stride=999, out=None) == (E, T_OUT)   # one row: no stride rule
    assert call(raw, inp=None, in_stride=0, out=None) == (E, T_OUT)                   # no input: in_stride unused
    assert call(raw, out=4096, **ALL_NULL) == (E, T_NOTHING)                          # in place, equal strides
    assert call(raw, inp=None, gain=None, fcw=None, phase=None, out=None) == (E, T_OUT)  # noise only is work
    if raw:
        for f in (4, -1):
            assert call(raw, fmt=f) == (E, T_FORMAT)
        assert call(raw, out=8194, fmt=_capi.LORA_IQ_CS16) == (E, T_OUT_ALIGN)        # cs16: 4 bytes
        for f in (_capi.LORA_IQ_CS8, _capi.LORA_IQ_CU8):                              # 8-bit formats: 2 bytes
            assert call(raw, out=8193, fmt=f) == (E, T_OUT_ALIGN)
            assert call(raw, out=8194, fmt=f, **ALL_NULL) == (E, T_NOTHING)
        assert call(raw, out=8196, fmt=_capi.LORA_IQ_CS16, **ALL_NULL) == (E, T_NOTHING)
    else:
        assert call(raw, out=8196) == (E, T_OUT_ALIGN)                                # complex64: 8 bytes
        assert call(raw, out=8200, **ALL_NULL) == (E, T_NOTHING)


@pytest.mark.parametrize("raw", [False, True])
def test_refusals_come_in_the_headers_order(raw):
    """A call that breaks two rules at once is refused with the earlier rule's text, for every
    pair of rules that can be broken together."""
    E = _capi.LORA_EINVAL
    call = caller()
    order = [t for t in ORDER if raw or t != T_FORMAT]
    pairs = 0
    for i, first in enumerate(order):
        for later in order[i + 1:]:
            kw = dict(BREAK[later])
            kw.update(BREAK[first])
            if any(kw[k] != v for k, v in BREAK[later].items()):
                continue  # the two rules need different values of one argument
            if kw.get("inp", 0) is None and first == T_IN_STRIDE:
                continue  # with no input its stride is not looked at
            if "inp" in BREAK[later] and first == T_INPLACE:
                continue  # another input is not `out`
            assert call(raw, **kw) == (E, first), (first, later)
            pairs += 1
    assert pairs >= 40


@pytest.mark.parametrize("raw", [False, True])
def test_nothing_to_do_makes_no_hip_call(raw):
    """rows == 0 or row_len == 0 is not an error, needs no pointer and makes no HIP call (on this
    machine one would fail): row_len comes back."""
    call = caller()
    none = dict(ALL_NULL, inp=None, out=None)
    assert call(raw, rows=0)[0] == 1000
    assert call(raw, rows=0, **none)[0] == 1000
    assert call(raw, row_len=0, in_stride=0, out_stride=0)[0] == 0
    assert call(raw, row_len=0, in_stride=0, out_stride=0, **none)[0] == 0


def test_stream_exports_and_host_checks():
    import torch

    import lora_phy_amd as amd
    from lora_phy_amd import stream

    for name in ("impair", "cfo_word", "noise_sigma"):
        assert name in stream.__all__ and name in amd.__all__ and getattr(amd, name) is getattr(stream, name)
    # cfo_word: to nearest, wrapped into int32
    assert stream.cfo_word(0.0) == 0 and stream.cfo_word(0.25) == 1 << 30 and stream.cfo_word(-0.25) == -(1 << 30)
    assert stream.cfo_word(0.5) == stream.cfo_word(-0.5) == -(1 << 31)
    assert stream.cfo_word(1.0) == 0 and stream.cfo_word(1.25) == 1 << 30
    assert stream.cfo_word(1.4 / (1 << 32)) == 1 and stream.cfo_word(1.6 / (1 << 32)) == 2
    assert stream.cfo_word(-1.6 / (1 << 32)) == -2
    for c in (0.0, 0.25, -0.25, 0.5, 1.25, 0.123456789, -0.49):
        assert stream.cfo_word(c) == ic.cfo_word(c)
    # noise_sigma: awgn.sweep_chain's convention
    assert stream.noise_sigma(0.0) == pytest.approx(1 / math.sqrt(2), rel=1e-15)
    assert stream.noise_sigma(20.0, 3.0) == pytest.approx(0.3 / math.sqrt(2), rel=1e-15)
    x = torch.zeros(16, dtype=torch.complex64)
    with pytest.raises(ValueError):
        stream.impair(x, sigma=1.0, snr_db=3.0)
    with pytest.raises(ValueError):
        stream.impair(x, sigma=1.0, scale=128.0)
    with pytest.raises(TypeError):
        stream.impair(x, sigma=1.0, dtype=torch.int32)
    with pytest.raises(TypeError):
        stream.impair(x, sigma=1.0)             # a CPU tensor: there is no CPU fallback
    with pytest.raises(ValueError):
        stream.impair(None, sigma=1.0)          # noise only needs a length
    with pytest.raises(TypeError):
        stream.impair(None, sigma=1.0, length=8, device="cpu")
