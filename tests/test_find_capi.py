"""CPU: the device frame finder's entry (lora_find_frames_batch, csrc/lora_find.hip) is declared,
exported and bound, and refuses every bad argument of the header's list before any HIP call -
seen on a machine with no GPU, where a HIP call could only fail otherwise.  The Python wrappers
(lora_phy_amd.stream.find_frames_device, receive_device, receive_wideband_device) refuse what the
entry cannot know: a bandwidth other than 125 kHz, and a `first` tensor of the wrong shape or
dtype.  tests/test_gpu_find.py holds the results against the host model."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

import lora_phy_amd as amd
from lora_phy_amd import _capi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "lora_mi355x.h")
NAMES = {"lora_find_frames_tile": [],
         "lora_find_frames_batch": [C.POINTER(_capi.FindParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                    C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p]}
E = _capi.LORA_EINVAL


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
    assert list(fn.argtypes or []) == NAMES[name]


def test_params_struct_matches_the_header():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\}\s*lora_find_params;", text).group(1)
    assert re.findall(r"(\w+)\s*;", body) == [f for f, _ in _capi.FindParams._fields_]


def test_the_exported_tile_is_the_kernels():
    assert _capi.lib().lora_find_frames_tile() == _capi.FIND_TILE
    assert _capi.FIND_TILE % 64 == 0


def params(sf=7, osr=1, sync=0x12, thresh_db=0.0, hop=32, frame_symbols=6, device=0):
    return _capi.FindParams(sf, osr, sync, thresh_db, hop, frame_symbols, device)


def call(p="default", metrics=(8, 8, 8), rows=1, W=100, stride=100, first=None, row_len=4000, capacity=3,
         starts=8, count=8, end=8):
    """The entry with dummy non-NULL pointers (never dereferenced on the host): every argument is
    valid unless the test says otherwise."""
    prm = params() if p == "default" else p
    return _capi.lib().lora_find_frames_batch(C.byref(prm) if prm is not None else None, *metrics, rows, W, stride,
                                              first, row_len, capacity, starts, count, end, None)


def test_entry_refuses_null_pointers_with_work_to_do():
    assert call(p=None) == E and _capi.lib().lora_last_error().decode()
    assert call(count=None) == E and call(end=None) == E
    assert call(starts=None) == E
    for i in range(3):
        m = [8, 8, 8]
        m[i] = None
        assert call(metrics=tuple(m)) == E, i
    assert call(p=None, rows=0) == E  # nothing to do still needs its parameters


def test_entry_refuses_bad_geometry():
    for sf in (5, 13, 0):
        assert call(p=params(sf=sf, hop=(1 << sf) // 4 or 1)) == E, sf
    assert call(p=params(osr=0)) == E
    assert call(p=params(hop=0)) == E and call(p=params(hop=-32)) == E
    assert call(p=params(hop=48)) == E        # does not divide step = 128
    assert call(p=params(hop=128)) == E       # step / hop = 1
    assert call(p=params(hop=256)) == E
    assert call(p=params(osr=2, hop=256)) == E
    assert call(p=params(frame_symbols=-1)) == E


def test_entry_refuses_bad_sizes():
    assert call(rows=-1) == E and call(W=-1) == E and call(stride=-1) == E
    assert call(row_len=-1) == E and call(capacity=-1) == E
    assert call(rows=2, W=100, stride=99) == E
    assert call(W=1 << 31, stride=1 << 31) == E
    assert call(rows=1 << 31) == E


def test_no_launch_needs_no_gpu():
    """rows == 0 is no launch: the one valid call that can be made without a device."""
    assert call(rows=0, metrics=(None, None, None), starts=None, count=None, end=None) == 0


def cpu_metrics(R=None, W=64):
    shape = (W,) if R is None else (R, W)
    return amd.DetectMetrics(torch.zeros(shape), torch.zeros(shape), None, torch.zeros(shape, dtype=torch.uint16))


def test_find_frames_device_refuses_what_the_host_finder_refuses():
    find = amd.stream.find_frames_device
    m = cpu_metrics()
    with pytest.raises(ValueError):
        find(m, 32, 7, 1, 6, bw=250000)
    for sf in (5, 13):
        with pytest.raises(ValueError):
            find(m, (1 << sf) // 4, sf, 1, 6)
    for hop in (48, 128, 256, 0, -32):
        with pytest.raises(ValueError):
            find(m, hop, 7, 1, 6)
    with pytest.raises(ValueError):
        find(m, 32, 7, 1, -1)


def test_find_frames_device_refuses_a_bad_first_tensor():
    find = amd.stream.find_frames_device
    with pytest.raises(ValueError):
        find(cpu_metrics(3), 32, 7, 1, 6, first=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError):
        find(cpu_metrics(3), 32, 7, 1, 6, first=torch.zeros((3, 1), dtype=torch.int64))
    with pytest.raises(ValueError):
        find(cpu_metrics(), 32, 7, 1, 6, first=torch.zeros(2, dtype=torch.int64))
    for dt in (torch.int32, torch.float32):
        with pytest.raises(TypeError):
            find(cpu_metrics(3), 32, 7, 1, 6, first=torch.zeros(3, dtype=dt))
    with pytest.raises(ValueError):
        find(cpu_metrics(), 32, 7, 1, 6, first=-1)


def test_there_is_no_cpu_fallback():
    """Valid arguments on CPU tensors are a TypeError, not a host computation."""
    with pytest.raises(TypeError):
        amd.stream.find_frames_device(cpu_metrics(2), 32, 7, 1, 6)
    with pytest.raises(TypeError):
        amd.stream.find_frames_device(cpu_metrics(2), 32, 7, 1, 6, first=torch.zeros(2, dtype=torch.int64))


def fake_plan(sf=7, bw=125000, dechirp=True):
    plan = object.__new__(amd.DemodPlan)  # no GPU is needed to reach the argument checks
    plan.device, plan.sf, plan.osr, plan.bw, plan.dechirp = torch.device("cuda", 0), sf, 1, bw, dechirp
    plan.N = plan.step = 1 << sf
    plan._h = None  # (close() in __del__ finds nothing to destroy)
    return plan


def test_receive_device_wrappers_refuse_bad_plans_and_hops():
    x = torch.zeros(4000, dtype=torch.complex64)
    chan = object.__new__(amd.stream.Channelizer)
    chan.device = torch.device("cuda", 0)
    for rx in (lambda plan, **kw: amd.stream.receive_device(plan, x, 6, **kw),
               lambda plan, **kw: amd.stream.receive_wideband_device(plan, chan, x, 6, **kw)):
        with pytest.raises(ValueError):
            rx(fake_plan(bw=250000))
        with pytest.raises(ValueError):
            rx(fake_plan(dechirp=False))
        with pytest.raises(ValueError):
            rx(fake_plan(sf=5))
        with pytest.raises(ValueError):
            rx(fake_plan(sf=13))
        for hop in (48, 128):
            with pytest.raises(ValueError):
                rx(fake_plan(), hop=hop)
    with pytest.raises(TypeError):
        amd.stream.receive_device(fake_plan(), x, 6)  # a CPU stream: no fallback


def test_new_names_are_public():
    for name in ("FoundFrames", "StreamFrames", "find_frames_device", "receive_device", "receive_wideband_device"):
        assert name in amd.stream.__all__ and getattr(amd.stream, name)
    assert amd.LoRaDemod.work_stream_device and amd.LoRaDemod.work_wideband_device
