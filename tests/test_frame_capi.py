"""CPU: the self-describing frame's C-ABI (lora_frame_symbols, lora_encode_frame_batch,
lora_decode_frame_batch), the frame gather's (lora_gather_frames_batch) and the two finder
entries' (lora_find_candidates_batch, lora_select_frames_batch) are declared, exported and
bound, and reject bad parameters before any HIP call (no GPU is needed: every call here returns
from its validation).  The kernels are checked by tests/test_gpu_frame.py and
tests/test_gpu_frames_stream.py."""
import ctypes as C
import os
import re
import subprocess

import pytest

from lora_phy_amd import _capi
from tests import frame_checker as fc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "lora_mi355x.h")

FRAME = ("lora_frame_symbols", "lora_encode_frame_batch", "lora_decode_frame_batch", "lora_gather_frames_batch",
         "lora_find_candidates_batch", "lora_select_frames_batch")
EINVAL = _capi.LORA_EINVAL
P = 0x1000  # a non-NULL, 16-byte aligned pointer value; validation returns before any buffer is touched


def test_header_declares_and_library_exports_the_entries():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"^[A-Za-z_][\w\s\*]*?\b(lora_\w+)\s*\(", text, flags=re.M))
    assert set(FRAME) <= declared
    assert set(FRAME) <= set(_capi.EXPORTED_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert set(FRAME) <= exported


def test_header_cites_the_reference_and_states_the_layout():
    text = open(HEADER).read()
    for name in FRAME[:4]:  # (the finder's rule is the library's own: the reference has none to cite)
        i = text.index(name + "(")
        comment = text[text.rindex("/*", 0, i):i]
        assert re.search(r"\.(cpp|hpp):\d+", comment), name
    for code, name in enumerate(("OK", "HEADER", "SHORT", "CRC")):
        assert re.search(r"#define LORA_FRAME_%s %d\b" % (name, code), text), name
    assert (fc.OK, fc.HEADER, fc.SHORT, fc.CRC) == (0, 1, 2, 3)


def test_ctypes_signatures_are_set():
    lib = _capi.lib()
    nargs = {"lora_frame_symbols": 4, "lora_encode_frame_batch": 13, "lora_decode_frame_batch": 17,
             "lora_gather_frames_batch": 10, "lora_find_candidates_batch": 12, "lora_select_frames_batch": 16}
    for name, n in nargs.items():
        fn = getattr(lib, name)
        assert fn.restype is C.c_int64, name
        assert fn.argtypes is not None and len(fn.argtypes) == n, name


def _encode(sf=7, rdd=1, crc=1, pay=P, frames=1, n=16, pstride=16, nbytes=None, sym=P, sstride=38, nsym=None):
    return _capi.lib().lora_encode_frame_batch(sf, rdd, crc, pay, frames, n, pstride, nbytes, sym, sstride, nsym, 0,
                                               None)


def _decode(sf=7, sym=P, frames=1, S=38, sstride=38, avail=None, status=P, pay=P, n=16, pstride=16):
    return _capi.lib().lora_decode_frame_batch(sf, sym, frames, S, sstride, avail, status, None, None, None, None,
                                               None, pay, n, pstride, 0, None)


def _gather(flat=P, total=100, at=P, length=P, slots=2, cut=10, out=P, ostride=10):
    return _capi.lib().lora_gather_frames_batch(flat, total, at, length, slots, cut, out, ostride, 0, None)


def _candidates(sf=7, osr=1, hop=32, prm=True, power=P, rows=1, W=100, stride=100, row_len=3296, cap=4, starts=P,
                count=P):
    p = _capi.FindParams(sf, osr, 0x12, 0.0, hop, 0, 0)
    return _capi.lib().lora_find_candidates_batch(C.byref(p) if prm else None, power, power, power, rows, W, stride,
                                                  row_len, cap, starts, count, None)


def _select(cand=P, status=P, nsym=P, rows=1, slots=4, row_len=5000, step=128, max_symbols=40, cap=3, starts=P,
            out_nsym=P, count=P, end=P):
    return _capi.lib().lora_select_frames_batch(cand, status, nsym, rows, slots, None, row_len, step, max_symbols, cap,
                                                starts, out_nsym, count, end, 0, None)


def _symbols(*a):
    return _capi.lib().lora_frame_symbols(*a)


REJECTED = [
    # sf outside 7..12 (SF6 has no header block), rdd outside 0..4, nbytes outside 0..255, crc outside {0, 1}
    ("symbols sf 6", lambda: _symbols(6, 1, 4, 1)),
    ("symbols sf 13", lambda: _symbols(13, 1, 4, 1)),
    ("symbols rdd -1", lambda: _symbols(7, -1, 4, 1)),
    ("symbols rdd 5", lambda: _symbols(7, 5, 4, 1)),
    ("symbols nbytes -1", lambda: _symbols(7, 1, -1, 1)),
    ("symbols nbytes 256", lambda: _symbols(7, 1, 256, 1)),
    ("symbols crc 2", lambda: _symbols(7, 1, 4, 2)),
    ("encode sf 6", lambda: _encode(sf=6)),
    ("encode sf 13", lambda: _encode(sf=13)),
    ("encode rdd -1", lambda: _encode(rdd=-1)),
    ("encode rdd 5", lambda: _encode(rdd=5)),
    ("encode crc 2", lambda: _encode(crc=2)),
    ("encode max_bytes 256", lambda: _encode(n=256, pstride=256, sstride=4096)),
    ("encode max_bytes -1", lambda: _encode(n=-1)),
    ("decode sf 6", lambda: _decode(sf=6)),
    ("decode sf 13", lambda: _decode(sf=13)),
    ("decode max_bytes 256", lambda: _decode(n=256, pstride=256)),
    ("decode max_bytes -1", lambda: _decode(n=-1)),
    # negative sizes
    ("encode negative frames", lambda: _encode(frames=-1)),
    ("decode negative frames", lambda: _decode(frames=-1)),
    ("decode negative sym_count", lambda: _decode(S=-1)),
    ("decode sym_count 2^31", lambda: _decode(S=1 << 31, sstride=1 << 31)),
    ("gather negative total", lambda: _gather(total=-1)),
    ("gather negative slots", lambda: _gather(slots=-1)),
    ("gather negative cut", lambda: _gather(cut=-1)),
    # a stride smaller than the row
    ("encode payload_stride", lambda: _encode(pstride=15)),
    ("encode sym_stride", lambda: _encode(sstride=37)),
    ("decode sym_stride", lambda: _decode(sstride=37)),
    ("decode payload_stride", lambda: _decode(pstride=15)),
    ("gather out_stride", lambda: _gather(ostride=9)),
    # a NULL required pointer
    ("encode null payload", lambda: _encode(pay=None)),
    ("encode null symbols", lambda: _encode(sym=None)),
    ("decode null symbols", lambda: _decode(sym=None)),
    ("gather null flat", lambda: _gather(flat=None)),
    ("gather null at", lambda: _gather(at=None)),
    ("gather null len", lambda: _gather(length=None)),
    ("gather null out", lambda: _gather(out=None)),
    # the finder entries: geometry as lora_find_frames_batch's, NULL buffers, negative sizes
    ("candidates null params", lambda: _candidates(prm=False)),
    ("candidates sf 5", lambda: _candidates(sf=5)),
    ("candidates sf 13", lambda: _candidates(sf=13)),
    ("candidates osr 0", lambda: _candidates(osr=0)),
    ("candidates hop 0", lambda: _candidates(hop=0)),
    ("candidates hop not dividing step", lambda: _candidates(hop=48)),
    ("candidates hop = step", lambda: _candidates(hop=128)),
    ("candidates negative rows", lambda: _candidates(rows=-1)),
    ("candidates negative W", lambda: _candidates(W=-1)),
    ("candidates W 2^31", lambda: _candidates(W=1 << 31, stride=1 << 31)),
    ("candidates negative row_len", lambda: _candidates(row_len=-1)),
    ("candidates negative capacity", lambda: _candidates(cap=-1)),
    ("candidates stride below W", lambda: _candidates(rows=2, stride=99)),
    ("candidates null count", lambda: _candidates(count=None)),
    ("candidates null starts", lambda: _candidates(starts=None)),
    ("candidates null metrics", lambda: _candidates(power=None)),
    ("select negative rows", lambda: _select(rows=-1)),
    ("select negative slots", lambda: _select(slots=-1)),
    ("select slots 2^31", lambda: _select(slots=1 << 31)),
    ("select negative row_len", lambda: _select(row_len=-1)),
    ("select negative capacity", lambda: _select(cap=-1)),
    ("select step 0", lambda: _select(step=0)),
    ("select negative max_symbols", lambda: _select(max_symbols=-1)),
    ("select null count", lambda: _select(count=None)),
    ("select null end", lambda: _select(end=None)),
    ("select null starts", lambda: _select(starts=None)),
    ("select null nsym out", lambda: _select(out_nsym=None)),
    ("select null candidates", lambda: _select(cand=None)),
    ("select null status", lambda: _select(status=None)),
    ("select null nsym", lambda: _select(nsym=None)),
    # the gather's alignment: 8 bytes for the stream, 16 for the output and each of its rows
    ("gather flat misaligned", lambda: _gather(flat=P + 4)),
    ("gather out misaligned", lambda: _gather(out=P + 8)),
    ("gather odd out_stride", lambda: _gather(ostride=11)),
]


@pytest.mark.parametrize("what,call", REJECTED, ids=[r[0] for r in REJECTED])
def test_validation_precedes_any_hip_call(what, call):
    lib = _capi.lib()
    assert call() == EINVAL, what
    assert lib.lora_last_error().decode(), what


def test_nothing_to_do_is_a_no_op_returning_the_per_frame_count():
    assert _encode(pay=None, sym=None, frames=0) == 38
    assert _decode(sym=None, pay=None, status=None, frames=0) == 0   # a NULL payload: header-only mode
    assert _decode(sym=None, frames=0) == 16
    assert _decode(pay=None, status=None) == 0                       # no output asked for
    assert _gather(flat=None, at=None, length=None, out=None, slots=0) == 10
    assert _candidates(power=None, starts=None, count=None, rows=0) == 0
    assert _select(cand=None, status=None, nsym=None, starts=None, out_nsym=None, count=None, end=None, rows=0) == 0
    assert _gather(flat=None, at=None, length=None, out=None, cut=0, ostride=0) == 0


@pytest.mark.parametrize("sf", range(7, 13))
def test_frame_symbols_equals_the_checker(sf):
    lib = _capi.lib()
    for rdd in range(5):
        for crc in (0, 1):
            for n in (0, 1, 2, 3, 4, 5, sf, 16, 17, 254, 255):
                want = fc.frame_symbols(sf, n, rdd, crc)
                assert lib.lora_frame_symbols(sf, rdd, n, crc) == want, (sf, rdd, crc, n)
    assert lib.lora_frame_symbols(7, 1, 16, 1) == 38 and lib.lora_frame_symbols(12, 4, 255, 1) == 352


def test_wrappers_have_no_cpu_fallback():
    import torch

    from lora_phy_amd import codec, stream

    pay = torch.zeros((2, 8), dtype=torch.uint8)
    sym = torch.zeros((2, 24), dtype=torch.uint16)
    with pytest.raises(TypeError):
        codec.encode_frame(pay, None, 7, "4/8")
    with pytest.raises(TypeError):
        codec.decode_frame(sym, 7)
    with pytest.raises(TypeError):
        codec.decode_header(sym, 7)
    with pytest.raises(TypeError):
        stream.gather_frames_device(torch.zeros(64, dtype=torch.complex64), torch.zeros(1, dtype=torch.int64),
                                    torch.zeros(1, dtype=torch.int64), 8)


def test_python_arithmetic_equals_the_library():
    from lora_phy_amd import codec

    assert (codec.FRAME_OK, codec.FRAME_HEADER, codec.FRAME_SHORT, codec.FRAME_CRC) == (0, 1, 2, 3)
    assert codec.frame_symbols(7, "4/5", 16) == 38 and codec.frame_symbols(12, 4, 0, crc=False) == 8
    with pytest.raises(_capi.LoraError):
        codec.frame_symbols(6, 1, 4)
    # frame_capacity: the longest payload whose frame (rate 4/4, no CRC) fits the symbols
    for sf in range(7, 13):
        for S in (0, 7, 8, 11, 12, 13, 40, 200, 400):
            cap = codec.frame_capacity(sf, S)
            if S < 8:
                assert cap == 0
                continue
            assert fc.frame_symbols(sf, cap, 0, 0) <= S
            assert cap == 255 or fc.frame_symbols(sf, cap + 1, 0, 0) > S


def test_the_blocks_are_exported():
    import lora_phy_amd

    assert hasattr(lora_phy_amd.LoRaMod, "work_frame")
    for name in ("gather_frames_device", "find_candidates_device", "select_frames_device", "receive_frames_device",
                 "receive_wideband_frames_device", "StreamPackets"):
        assert name in lora_phy_amd.stream.__all__ and hasattr(lora_phy_amd.stream, name), name
    assert hasattr(lora_phy_amd.LoRaDemod, "work_packets_device")
    assert hasattr(lora_phy_amd.LoRaDemod, "work_wideband_packets_device")
