"""CPU: lora_demod_spec_trace is declared, exported and bound, and refuses bad arguments with
the documented codes and texts, in the documented order, before it touches the plan (no GPU is
needed: every call here returns from its validation).  The refusals that need a plan - a last
call that did not take the pipeline, a small symbol, workspace or list capacity - and the copy
itself are in tests/test_gpu_cert.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from lora_phy_amd import _capi, demod

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "lora_mi355x.h")
NAME = "lora_demod_spec_trace"
EINVAL, ERANGE = _capi.LORA_EINVAL, _capi.LORA_ERANGE
P = 0x1000  # a non-NULL pointer value; validation returns before any pointer is followed


def test_header_declares_library_exports_and_binding_is_set():
    text = open(HEADER).read()
    bare = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"^[A-Za-z_][\w\s\*]*?\b(lora_\w+)\s*\(", bare, flags=re.M))
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert NAME in declared and NAME in _capi.EXPORTED_SYMBOLS and NAME in exported
    fn = getattr(_capi.lib(), NAME)
    assert fn.restype is C.c_int64 and len(fn.argtypes) == 7
    # the header comment says what stays readable after k_spec_fix in each of the three pipelines
    i = text.index(NAME + "(")
    comment = text[text.rindex("/*", 0, text.rindex("typedef struct lora_spec_frame", 0, i)):i]
    for word in ("LEGACY", "API", "RAW", "k_spec_fix", "0xFFFFFFFF", "LORA_ERANGE"):
        assert word in comment, word


def test_structs_match_the_header():
    """lora_spec_frame is 32 bytes (FrameParams), lora_spec_trace_out five pointers and three
    int64 capacities, in the header's order."""
    assert np.dtype(demod.SPEC_FRAME_DTYPE).itemsize == 32
    text = open(HEADER).read()
    body = text[text.index("typedef struct lora_spec_trace_out {"):text.index("} lora_spec_trace_out;")]
    names = re.findall(r"\*\s*(\w+);", body) + re.findall(r"(\w+_cap)\b", body.split("int64_t")[-1])
    assert names == [n for n, _ in _capi.SpecTraceOut._fields_]
    assert C.sizeof(_capi.SpecTraceOut) == 5 * C.sizeof(C.c_void_p) + 3 * 8


def _out(fp_spec=P, fp=P, max_slot=P, entries=P, lst=P, frame_cap=4, sym_cap=1 << 20, list_cap=1 << 20):
    return _capi.SpecTraceOut(fp_spec, fp, max_slot, entries, lst, frame_cap, sym_cap, list_cap)


def _trace(plan=P, ws=P, ws_bytes=1 << 30, frames=4, frame_len=1024, out=None, null_out=False):
    o = _out() if out is None else out
    return _capi.lib().lora_demod_spec_trace(plan, ws, ws_bytes, frames, frame_len, None if null_out else C.byref(o),
                                             None)


# in the entry's order: each case passes every check before its own
REJECTED = [
    ("null plan", lambda: _trace(plan=None, frames=-1), EINVAL, "null argument"),
    ("null workspace", lambda: _trace(ws=None, frames=-1), EINVAL, "null argument"),
    ("null out", lambda: _trace(null_out=True, frames=-1), EINVAL, "null argument"),
    ("no frames", lambda: _trace(frames=0, out=_out(fp=None)), EINVAL, "bad frames / frame_len"),
    ("negative frames", lambda: _trace(frames=-1, out=_out(fp=None)), EINVAL, "bad frames / frame_len"),
    ("negative frame_len", lambda: _trace(frame_len=-1, out=_out(fp=None)), EINVAL, "bad frames / frame_len"),
    ("null fp_spec", lambda: _trace(out=_out(fp_spec=None, frame_cap=0)), EINVAL, "null output buffer"),
    ("null fp", lambda: _trace(out=_out(fp=None, frame_cap=0)), EINVAL, "null output buffer"),
    ("null max_slot", lambda: _trace(out=_out(max_slot=None, frame_cap=0)), EINVAL, "null output buffer"),
    ("null entries", lambda: _trace(out=_out(entries=None, frame_cap=0)), EINVAL, "null output buffer"),
    ("null list", lambda: _trace(out=_out(lst=None, frame_cap=0)), EINVAL, "null output buffer"),
    ("frame_cap", lambda: _trace(out=_out(frame_cap=3)), ERANGE, "frame capacity too small"),
]


@pytest.mark.parametrize("what,call,code,text", REJECTED, ids=[r[0] for r in REJECTED])
def test_validation_precedes_any_use_of_the_plan(what, call, code, text):
    """Each case also carries the NEXT check's fault (a negative frame count behind a null
    argument, a null buffer behind it, a small frame capacity behind that), so the code and
    text returned show the order of the checks."""
    assert call() == code, what
    assert _capi.lib().lora_last_error().decode() == text, what


def test_wrapper_needs_a_run():
    import lora_phy_amd as amd

    plan = object.__new__(amd.DemodPlan)  # no GPU is needed to reach the check
    plan._h = None  # (close() in __del__ finds nothing to destroy)
    with pytest.raises(RuntimeError):
        amd.DemodPlan.spec_trace(plan)
