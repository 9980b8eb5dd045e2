"""CPU: the sliding-scan entry points (lora_detect_scan_windows, lora_detect_scan_batch) are
declared, exported and bound, and refuse bad arguments before any HIP call.  A plan cannot be
made without a GPU, so here every refusal is seen with a NULL plan, alone and beside each bad
argument; tests/test_gpu_scan.py repeats the bad arguments, and the window arithmetic of the
C function, with a real plan.  The window count's formula itself is checked here on the host
model the GPU tests compare against."""
import ctypes as C
import os
import re
import subprocess

import pytest

from lora_phy_amd import _capi
from tests import scan_checker as sc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "lora_mi355x.h")
NAMES = {"lora_detect_scan_windows": [C.c_void_p, C.c_int64, C.c_int64],
         "lora_detect_scan_batch": [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64,
                                    C.POINTER(_capi.SymbolMetrics), C.c_void_p]}


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
    # the header comment cites the reference lines, like its neighbours
    i = text.index(name + "(")
    assert "LoRaDetector.hpp:39-74" in text[text.rindex("/*", 0, i):i]


def test_scan_windows_refuses_a_null_plan_and_bad_arguments():
    lib = _capi.lib()
    E = _capi.LORA_EINVAL
    assert lib.lora_detect_scan_windows(None, 1024, 32) == E and lib.lora_last_error().decode()
    assert lib.lora_detect_scan_windows(None, -1, 32) == E
    assert lib.lora_detect_scan_windows(None, 1024, 0) == E
    assert lib.lora_detect_scan_windows(None, 1024, -5) == E


def test_window_count_formula():
    step, hop = 128, 32
    assert sc.scan_windows(step - 1, step, hop) == 0
    assert sc.scan_windows(0, step, hop) == 0
    assert sc.scan_windows(step, step, hop) == 1
    assert sc.scan_windows(step + hop - 1, step, hop) == 1
    assert sc.scan_windows(step + hop, step, hop) == 2
    assert sc.scan_windows(step + 5, step, step + 5) == 1  # hop > step
    assert sc.scan_windows(2 * step + 5, step, step + 5) == 2


def test_scan_batch_refuses_before_any_hip_call():
    """NULL plan, NULL out, and a NULL plan beside each bad argument of the header's list: all
    LORA_EINVAL with a message, on a machine with no GPU (so no HIP call was needed)."""
    lib = _capi.lib()
    E = _capi.LORA_EINVAL
    m = _capi.SymbolMetrics(None, None, None, None, 0)

    def call(plan=None, iq=None, rows=1, row_len=1024, row_stride=1024, hop=32, out=C.byref(m)):
        return lib.lora_detect_scan_batch(plan, iq, rows, row_len, row_stride, hop, out, None)

    assert call() == E and lib.lora_last_error().decode()
    assert call(out=None) == E
    assert call(rows=0, row_len=0, row_stride=0) == E       # nothing to do still needs a plan
    assert call(rows=-1) == E and call(row_len=-1) == E and call(row_stride=-1) == E
    assert call(hop=0) == E and call(hop=-3) == E
    assert call(row_len=1 << 31, row_stride=1 << 31) == E
    assert call(rows=2, row_stride=1023) == E
    m.stride = -1
    assert call() == E
    m.stride = 0
    assert call(rows=1 << 40) == E


def test_scan_has_no_cpu_fallback():
    import torch

    import lora_phy_amd as amd

    assert "stream" in amd.__all__ and amd.stream.receive and amd.stream.find_frames and amd.stream.extract_frames
    plan = object.__new__(amd.DemodPlan)  # no GPU is needed to reach the argument check
    plan.device, plan.mode, plan.step = torch.device("cuda", 0), "raw", 128
    with pytest.raises(TypeError):
        amd.DemodPlan.scan(plan, torch.zeros(256, dtype=torch.complex64), 32)
    with pytest.raises(TypeError):
        amd.DemodPlan.scan(plan, torch.zeros((2, 256), dtype=torch.complex64), 32)
    plan._h = None  # (close() in __del__ finds nothing to destroy)
