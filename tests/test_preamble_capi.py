"""CPU: the entry points of preambled frames are declared, exported and bound; every LORA_EINVAL
case is refused before any HIP call (seen on a machine with no GPU: a NULL plan beside each bad
argument for the scan, bad parameters for the finder and the selection); and
lora_preamble_tables - host arithmetic only - equals the host model bit for bit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from lora_phy_amd import _capi
from tests import preamble_checker as pc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "lora_mi355x.h")
NAMES = ("lora_preamble_tables", "lora_detect_scan_acc_windows", "lora_detect_scan_acc_batch",
         "lora_find_preamble_batch", "lora_select_preamble_batch")
E = _capi.LORA_EINVAL


@pytest.fixture(scope="module")
def O():
    from oracle.pyoracle import Oracle

    return Oracle()


@pytest.mark.parametrize("name", NAMES)
def test_header_declares_library_exports_and_binding_is_set(name):
    text = open(HEADER).read()
    bare = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert name in re.findall(r"^[A-Za-z_][\w\s\*]*?\b(lora_\w+)\s*\(", bare, flags=re.M)
    assert name in _capi.EXPORTED_SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert name in {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    fn = getattr(_capi.lib(), name)
    assert fn.restype is C.c_int64 and fn.argtypes


@pytest.mark.parametrize("sf,osr,bw,ampl,P", [(7, 1, 125000, 1.0, 8), (7, 2, 125000, 0.5, 4), (9, 1, 250000, 3.0, 6),
                                              (12, 1, 125000, 1.0, 5)])
def test_tables_equal_the_host_model(O, sf, osr, bw, ampl, P):
    lib = _capi.lib()
    step = (1 << sf) * osr
    assert lib.lora_preamble_tables(sf, osr, bw, ampl, P, None, None) == P * step
    pre = np.zeros(P * step, np.complex64)
    sfd = np.zeros(9 * step // 4, np.complex64)
    assert lib.lora_preamble_tables(sf, osr, bw, ampl, P, pre.ctypes.data, sfd.ctypes.data) == P * step
    wpre, wsfd = pc.tables_host(O, sf, osr, P, bw, ampl)
    assert np.array_equal(pre.view(np.uint32), wpre.view(np.uint32))
    assert np.array_equal(sfd.view(np.uint32), wsfd.view(np.uint32))
    # either pointer alone
    only = np.zeros_like(sfd)
    assert lib.lora_preamble_tables(sf, osr, bw, ampl, P, None, only.ctypes.data) == P * step
    assert np.array_equal(only.view(np.uint32), wsfd.view(np.uint32))


def test_tables_refuse_bad_arguments():
    lib = _capi.lib()

    def call(sf=7, osr=1, bw=125000, P=8):
        return lib.lora_preamble_tables(sf, osr, bw, 1.0, P, None, None)

    assert call() == 8 * 128 and call(osr=0) == 8 * 128
    assert call(sf=1) == E and lib.lora_last_error().decode()
    assert call(sf=13) == E and call(bw=100000) == E and call(P=3) == E and call(P=65) == E
    assert call(sf=2, osr=3) == 8 * 12  # (N >= 4, so a quarter symbol is always whole samples)


def test_scan_acc_refuses_before_any_hip_call():
    lib = _capi.lib()
    assert lib.lora_detect_scan_acc_windows(None, 1024, 32, 2) == E and lib.lora_last_error().decode()

    def call(plan=None, iq=None, rows=1, row_len=1024, row_stride=1024, hop=32, acc=2, ostride=0):
        return lib.lora_detect_scan_acc_batch(plan, iq, rows, row_len, row_stride, hop, acc, 0, None, None, None,
                                              ostride, None)

    assert call() == E and "null" in lib.lora_last_error().decode()
    # the checks that need no plan are made before the plan is looked at: their own message shows
    # that it was they who refused (the others, which read the plan's step, are seen with a real
    # plan in tests/test_gpu_scan_acc.py)
    for kw, text in (({"acc": 0}, "acc"), ({"acc": 9}, "acc"), ({"rows": -1}, "negative"), ({"row_len": -1}, "negative"),
                     ({"row_stride": -1}, "negative"), ({"ostride": -1}, "negative"), ({"hop": 0}, "hop")):
        assert call(**kw) == E and text in lib.lora_last_error().decode(), (kw, lib.lora_last_error())
    for kw in ({"row_len": 1 << 31, "row_stride": 1 << 31}, {"rows": 2, "row_stride": 1023}):
        assert call(**kw) == E, kw
    assert lib.lora_detect_scan_acc_windows(None, 1024, 32, 9) == E and "acc" in lib.lora_last_error().decode()


def params(sf=7, osr=1, hop=32, acc_up=6, tu=0.0, td=0.0, max_cfo=31, device=0):
    return _capi.PreambleParams(sf, osr, hop, acc_up, tu, td, max_cfo, device)


def test_find_preamble_refuses_before_any_hip_call():
    lib = _capi.lib()
    cnt = np.zeros(1, np.int32)

    def call(p=None, rows=1, Wu=0, Wd=0, us=0, ds=0, row_len=0, cap=0, count=cnt.ctypes.data, **kw):
        prm = params(**kw) if p is None else p
        return lib.lora_find_preamble_batch(C.byref(prm) if prm is not False else None, None, None, None, Wu, us, None,
                                            None, None, Wd, ds, rows, row_len, cap, None, None, count, None)

    assert call(p=False) == E and lib.lora_last_error().decode()
    for kw in ({"sf": 6}, {"sf": 13}, {"osr": 0}, {"osr": 1 << 17}, {"hop": 0}, {"hop": 48}, {"hop": 64},
               {"acc_up": 1}, {"acc_up": 9}, {"max_cfo": -1}, {"max_cfo": 32}):
        assert call(**kw) == E, kw
    for kw in ({"rows": -1}, {"Wu": -1}, {"Wd": -1}, {"us": -1}, {"ds": -1}, {"row_len": -1}, {"cap": -1},
               {"Wu": 1 << 31}, {"Wd": 1 << 31}, {"rows": 1 << 31}, {"rows": 2, "Wu": 5, "us": 4},
               {"rows": 2, "Wd": 5, "ds": 4}, {"count": None}, {"cap": 4}):
        assert call(**kw) == E, kw
    # windows to test and no metrics
    assert call(Wu=100, Wd=100, us=100, ds=100, row_len=10000) == E
    assert call(rows=0, count=None) == 0


def test_select_preamble_refuses_before_any_hip_call():
    lib = _capi.lib()
    one = np.zeros(1, np.int64)
    c32 = np.zeros(1, np.int32)

    def call(rows=1, slots=0, row_len=1000, step=128, tail=288, max_symbols=20, cap=0, count=c32.ctypes.data,
             end=one.ctypes.data):
        return lib.lora_select_preamble_batch(None, None, None, None, rows, slots, None, row_len, step, tail,
                                              max_symbols, cap, None, None, None, count, end, 0, None)

    for kw in ({"tail": -1}, {"rows": -1}, {"slots": -1}, {"row_len": -1}, {"cap": -1}, {"step": 0},
               {"max_symbols": -1}, {"rows": 1 << 31}, {"slots": 1 << 31}, {"count": None}, {"end": None},
               {"cap": 2}, {"slots": 3}):
        assert call(**kw) == E, kw
    assert lib.lora_last_error().decode()
    assert call(rows=0, count=None, end=None) == 0
    # cand_word and out_word go together: one without the other is refused before anything else
    # is looked at (host arrays stand in for the device pointers, which are never followed)
    slots = np.zeros(4, np.int64)
    w32 = np.zeros(4, np.int32)

    def words(word, out_word):
        return lib.lora_select_preamble_batch(slots.ctypes.data, word, w32.ctypes.data, w32.ctypes.data, 1, 4, None,
                                              100000, 128, 288, 20, 4, slots.ctypes.data, out_word, w32.ctypes.data,
                                              c32.ctypes.data, one.ctypes.data, 0, None)

    assert words(w32.ctypes.data, None) == E and "go together" in lib.lora_last_error().decode()
    assert words(None, w32.ctypes.data) == E and "go together" in lib.lora_last_error().decode()


def test_python_entries_have_no_cpu_fallback():
    import torch

    import lora_phy_amd as amd

    for name in ("find_preamble_device", "select_preamble_device", "receive_preamble_frames_device",
                 "receive_wideband_preamble_frames_device"):
        assert name in amd.stream.__all__ and callable(getattr(amd.stream, name))
    assert callable(amd.modulate_preamble) and callable(amd.preamble_tables)
    # the chain's default thresholds: the measured choice
    assert [amd.stream.preamble_threshold_db(sf) for sf in range(7, 13)] == [-10.0, -13.0, -16.0, -19.0, -22.0, -22.0]
    plan = object.__new__(amd.DemodPlan)
    plan.device, plan.mode, plan.step = torch.device("cuda", 0), "raw", 128
    with pytest.raises(TypeError):
        amd.DemodPlan.scan_acc(plan, torch.zeros(1024, dtype=torch.complex64), 32, 2)
    plan._h = None
    z = torch.zeros((1, 4), dtype=torch.int64)
    with pytest.raises(TypeError):
        amd.stream.select_preamble_device(z, z.int(), z.int(), z.int(), 128, 4000, 20)
    with pytest.raises(TypeError):
        amd.preamble_tables(7, device="cpu")
