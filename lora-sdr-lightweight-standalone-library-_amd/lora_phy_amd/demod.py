"""GPU demodulation: plan wrapper over lora_demod_batch and the LoRaDemod block.

The plan mirrors ``lora_demod_workspace`` (include/lora_phy/phy.hpp:170-185): it is
created once per (sf, osr, bw, window, dechirp, mode, device) and holds only constant
tables on the device.  IQ buffers are torch.complex64 CUDA tensors owned by the
caller; outputs are allocated with torch's caching allocator (no hipMalloc per call).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import threading
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import _capi

_WINDOWS = {"none": _capi.LORA_WINDOW_NONE, "hann": _capi.LORA_WINDOW_HANN,
            None: _capi.LORA_WINDOW_NONE, 0: _capi.LORA_WINDOW_NONE, 1: _capi.LORA_WINDOW_HANN}
_MODES = {"legacy": _capi.LORA_MODE_LEGACY, "api": _capi.LORA_MODE_API, "raw": _capi.LORA_MODE_RAW}
# include/lora_mi355x.h LORA_PRECISION_*: "exact" = bit-identical to the reference
# (default); "fast" = hardware sin/cos for the per-sample CFO rotation (stated tolerance).
_PRECISIONS = {"exact": 0, "fast": 1}


@dataclass
class DemodResult:
    """Per-frame results of one batched call (all tensors on the plan's device)."""

    symbols: torch.Tensor      # [F, S] uint16   (LoRaDemod.cpp:165-174)
    sync: torch.Tensor         # [F] uint8       (LoRaDemod.cpp:177-192)
    cfo: torch.Tensor          # [F] float32     (lora_metrics.cfo)
    time_offset: torch.Tensor  # [F] float32     (lora_metrics.time_offset)
    max_amp: torch.Tensor      # [F] float32     (LoRaDemod.cpp:59-67; 0 in API mode)


@dataclass
class DetectMetrics:
    """What LoRaDetector::detect returns for every whole symbol of every frame
    (LoRaDetector.hpp:39-74), column s = symbol s of the frame: the sync symbols are
    columns 0 and 1 and ``DemodResult.symbols`` equals ``index[:, 2:]``.  All tensors are on
    the plan's device; a field is None only where the caller's ``out=`` left it out."""

    power: Optional[torch.Tensor]      # [F, total] float32  the peak bin, dB          (:64)
    power_avg: Optional[torch.Tensor]  # [F, total] float32  every other bin, dB       (:60-63)
    f_index: Optional[torch.Tensor]    # [F, total] float32  fractional-bin offset     (:66-71)
    index: Optional[torch.Tensor]      # [F, total] uint16   the argmax bin            (:73)

    @property
    def snr_db(self) -> torch.Tensor:
        """``power - power_avg`` per symbol, a plain torch subtraction: the peak over
        everything else in the spectrum.  +inf where the floor is -inf (a noiseless tone on
        an exact bin); NaN for an all-zero window (both are -inf)."""
        return self.power - self.power_avg

    def frame_snr_db(self, first: int = 2) -> torch.Tensor:
        """Per frame, the mean of ``snr_db[:, first:]`` (default: the data symbols) - plain
        torch ops, accumulated in float64 and returned as float32.  NaN for a frame with no
        such symbol."""
        return self.snr_db[:, first:].double().mean(dim=1).float()


# lora_spec_frame (include/lora_mi355x.h) as a numpy record
SPEC_FRAME_DTYPE = [("cfo", "<f4"), ("time_offset", "<f4"), ("rate", "<f4"), ("scale", "<f4"),
                    ("t_off", "<i4"), ("scaled", "<i4"), ("reserved", "<i4", (2,))]


@dataclass
class SpecTrace:
    """``DemodPlan.spec_trace()``: the certification's inputs and verdicts of the last ``run``
    (lora_demod_spec_trace in include/lora_mi355x.h defines every field), host numpy arrays."""

    fp_spec: object   # [F] SPEC_FRAME_DTYPE  the offsets the symbol pass used
    fp: object        # [F] SPEC_FRAME_DTYPE  the exact offsets
    max_slot: object  # [F] uint32            float bits: the maximum outside the data windows
    margin: object    # [F, total] float32    |X1| - |X2| per symbol of the frame
    aux: object       # [F, total] uint32     data symbol: the window maximum's float bits; sync: the index
    rejected: object  # [K, 2] uint32         (frame, symbol of the frame | 0xFFFFFFFF = the sync pair)


def _stream_handle(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _require_cuda(t: torch.Tensor, name: str) -> None:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError(f"{name} must be a CUDA (HIP) torch tensor; the product path has no "
                        "CPU fallback")


def _check_buf(t: torch.Tensor, name: str, dtype: torch.dtype, device: torch.device, numel: int) -> None:
    """Everything the C library cannot check about a raw pointer: a wrong device, dtype,
    stride or length would be a GPU memory fault or silent corruption, not an error."""
    _require_cuda(t, name)
    if t.device != device:
        raise ValueError(f"{name} is on {t.device}, the plan is on {device}")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if numel > 0 and (not t.is_contiguous() or t.numel() < numel):
        raise ValueError(f"{name} must be contiguous with >= {numel} elements "
                         f"(got {t.numel()}, contiguous={t.is_contiguous()})")


def _check_iq(iq: torch.Tensor, device: torch.device) -> torch.Tensor:
    _require_cuda(iq, "iq")
    if iq.device != device:
        raise ValueError(f"iq is on {iq.device}, the plan is on {device}")
    if iq.dtype != torch.complex64:
        raise TypeError("iq must be complex64 (interleaved fp32 I/Q)")
    if iq.dim() == 1:
        iq = iq.unsqueeze(0)
    if iq.dim() != 2 or (iq.shape[1] > 1 and iq.stride(1) != 1) or (iq.shape[0] > 1 and iq.stride(0) < iq.shape[1]):
        raise ValueError("iq must be [frames, samples] with unit sample stride and non-overlapping rows")
    return iq


def _metric_outputs(out: Optional[DetectMetrics], F: int, total: int, dev: torch.device):
    """The (DetectMetrics, lora_symbol_metrics) pair of a call that writes [F, total] values:
    fresh tensors when ``out`` is None, else ``out``'s own after the checks the C library cannot
    make on raw pointers."""
    if out is None:
        out = DetectMetrics(*(torch.empty((F, total), dtype=dt, device=dev)
                              for dt in (torch.float32, torch.float32, torch.float32, torch.uint16)))
    given = []
    for name, dt in (("power", torch.float32), ("power_avg", torch.float32), ("f_index", torch.float32),
                     ("index", torch.uint16)):
        t = getattr(out, name)
        if t is None:
            continue
        _require_cuda(t, "out." + name)
        if t.dtype != dt:
            raise TypeError(f"out.{name} must be {dt}, got {t.dtype}")
        if (t.device != dev or t.dim() != 2 or t.shape[0] < F or t.shape[1] < total
                or (t.shape[1] > 1 and t.stride(1) != 1) or (F > 1 and t.stride(0) < total)):
            raise ValueError(f"out.{name} must be a {dt} [>={F}, >={total}] tensor on {dev} with unit "
                             "column stride and non-overlapping rows")
        given.append(t)
    # one row stride for the four outputs (lora_symbol_metrics.stride); a single row has none
    strides = {t.stride(0) for t in given} if F > 1 else set()
    if len(strides) > 1:
        raise ValueError("the tensors of out must share one row stride")
    m = _capi.SymbolMetrics(*(getattr(out, n).data_ptr() if getattr(out, n) is not None else None
                              for n in ("power", "power_avg", "f_index", "index")),
                            strides.pop() if strides else total)
    return out, m


class DemodPlan:
    """A device plan for one demodulator configuration (lora_demod_init equivalent)."""

    def __init__(self, sf: int, osr: int = 1, bw: int = 125000, window="none",
                 dechirp: bool = False, mode: str = "legacy", device=None, precision: str = "exact",
                 pipeline: Optional[str] = None):
        """``pipeline``: "spec" = the speculative single-read pipeline wherever it covers the
        configuration, "split" = always the three-launch exact path; None = the enclosing
        ``spec_pipeline`` block's choice on this thread, else the library default (spec,
        unless LORA_MI355X_SPEC=0 was set when the plan was created)."""
        if not torch.cuda.is_available():
            raise RuntimeError("lora_phy_amd needs a HIP GPU (torch.cuda.is_available() is False)")
        dev = torch.device("cuda", torch.cuda.current_device() if device is None else
                           torch.device(device).index or 0)
        self.device = dev
        self.sf, self.osr, self.bw = int(sf), int(osr) if osr else 1, int(bw)
        self.N = 1 << self.sf
        self.step = self.N * self.osr
        self.window = window
        self.dechirp = bool(dechirp)
        self.mode = mode
        if precision not in _PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(_PRECISIONS)}")
        self.precision = precision
        self._lib = _capi.lib()
        prm = _capi.DemodParams(self.sf, self.osr, self.bw, _WINDOWS[window], int(self.dechirp),
                                _MODES[mode], dev.index, _PRECISIONS[precision])
        h = C.c_void_p()
        _capi.check(self._lib.lora_demod_plan_create(C.byref(prm), C.byref(h)))
        self._h = h
        if pipeline is None:
            pipeline = getattr(_PIPELINE, "choice", None)
        if pipeline is not None:
            if pipeline not in ("spec", "split"):
                raise ValueError('pipeline must be "spec", "split" or None')
            _capi.check(self._lib.lora_demod_plan_set_pipeline(h, int(pipeline == "spec")))
        self.pipeline = pipeline
        # Workspaces per stream (two streams never share frame maxima / FrameParams);
        # ones used while a HIP graph was being captured are kept for the plan's lifetime,
        # since the graph replays with their addresses.
        self._ws: dict = {}
        self._ws_captured: list = []

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.lora_demod_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def symbols_per_frame(self, frame_len: int) -> int:
        return _capi.check(self._lib.lora_demod_symbols_per_frame(self._h, int(frame_len)))

    def last_kernels(self) -> set:
        """Kernels the last run() launched: {"spec", "estimate", "demod"} for the speculative
        single-read pipeline, {"frame_max", "estimate", "demod"} for the three-launch path
        (+"generic", "frame_max_wave")."""
        m = self._lib.lora_demod_last_kernels(self._h)
        return {k for k, b in _capi.KERNEL_BITS.items() if m & b}

    def spec_recomputed(self) -> int:
        """Data symbols the speculative pipeline has recomputed exactly on this plan (their
        certification margin was too small); synchronises the device."""
        return _capi.check(self._lib.lora_demod_spec_recomputed(self._h))

    def _workspace(self, frames: int, frame_len: int) -> torch.Tensor:
        need = self._lib.lora_demod_workspace_bytes(self._h, int(frames), int(frame_len))
        key = _stream_handle(self.device)
        ws = self._ws.get(key)
        if ws is None or ws.numel() < need:
            # allocated on (and stream-ordered with) the current stream, so dropping the
            # smaller one is safe for work already queued on it
            ws = torch.empty(max(need, 256), dtype=torch.uint8, device=self.device)
            self._ws[key] = ws
            if torch.cuda.is_current_stream_capturing():
                self._ws_captured.append(ws)
        return ws

    def run(self, iq: torch.Tensor, out: Optional[DemodResult] = None) -> DemodResult:
        """Demodulate a [F, L] (or [L]) complex64 CUDA tensor; one frame per row."""
        iq = _check_iq(iq, self.device)
        F, L = iq.shape
        S = self.symbols_per_frame(L)
        dev = self.device
        if out is None:
            out = DemodResult(
                symbols=torch.empty((F, max(S, 0)), dtype=torch.uint16, device=dev),
                sync=torch.empty(F, dtype=torch.uint8, device=dev),
                cfo=torch.empty(F, dtype=torch.float32, device=dev),
                time_offset=torch.empty(F, dtype=torch.float32, device=dev),
                max_amp=torch.zeros(F, dtype=torch.float32, device=dev))
        else:
            if S > 0:
                _require_cuda(out.symbols, "out.symbols")
                if (out.symbols.dtype != torch.uint16 or out.symbols.device != dev or out.symbols.dim() != 2
                        or out.symbols.shape[0] < F or out.symbols.shape[1] < S or out.symbols.stride(1) != 1):
                    raise ValueError(f"out.symbols must be a uint16 [>={F}, >={S}] tensor on {dev}")
            for name, dt in (("sync", torch.uint8), ("cfo", torch.float32), ("time_offset", torch.float32),
                             ("max_amp", torch.float32)):
                _check_buf(getattr(out, name), "out." + name, dt, dev, F)
        ws = self._workspace(F, L)
        o = _capi.DemodOutputs(out.symbols.data_ptr() if S > 0 else None,
                               out.symbols.stride(0) if S > 0 else 0,
                               out.sync.data_ptr(), out.cfo.data_ptr(), out.time_offset.data_ptr(),
                               out.max_amp.data_ptr())
        stride = iq.stride(0) if F > 1 else L
        st = _stream_handle(dev)
        _capi.check(self._lib.lora_demod_batch(self._h, iq.data_ptr(), F, L, stride, C.byref(o),
                                               ws.data_ptr(), ws.numel(), st))
        self._last_run = (F, L, ws, st)  # what spec_trace() reads back
        return out

    def spec_trace(self) -> SpecTrace:
        """What the speculative pipeline's certification saw and decided in the last ``run``
        (lora_demod_spec_trace), as numpy arrays on the host: a diagnostic for tests and tools.
        Synchronises the run's stream.  Raises when no ``run`` took the pipeline last."""
        import numpy as np

        last = getattr(self, "_last_run", None)
        if last is None:
            raise RuntimeError("run() has not run")
        F, L, ws, stream = last
        total = L // self.step
        fp_spec = np.zeros(F, SPEC_FRAME_DTYPE)
        fp = np.zeros(F, SPEC_FRAME_DTYPE)
        max_slot = np.zeros(F, np.uint32)
        entries = np.zeros((F, total, 2), np.uint32)
        # the most the certification can list: every symbol, and a sync pair per frame
        rejected = np.zeros((F * (total + 1), 2), np.uint32)
        o = _capi.SpecTraceOut(fp_spec.ctypes.data, fp.ctypes.data, max_slot.ctypes.data, entries.ctypes.data,
                               rejected.ctypes.data, F, F * total, len(rejected))
        n = _capi.check(self._lib.lora_demod_spec_trace(self._h, ws.data_ptr(), ws.numel(), F, L, C.byref(o),
                                                        stream))
        return SpecTrace(fp_spec, fp, max_slot, entries[:, :, 0].copy().view(np.float32), entries[:, :, 1].copy(),
                         rejected[:n].copy())

    def detect_metrics(self, iq: torch.Tensor, result: Optional[DemodResult] = None,
                       out: Optional[DetectMetrics] = None) -> DetectMetrics:
        """The detector's per-symbol outputs (lora_demod_metrics_batch) for the frames of a
        [F, L] (or [L]) complex64 CUDA tensor, laid out as for ``run``.

        ``result``: the ``DemodResult`` of ``run`` on the same frames - its cfo, time_offset
        and (legacy) max_amp rebuild each symbol's window; required for legacy / api plans,
        ignored for raw ones.  ``out``: a ``DetectMetrics`` whose tensors ([>= F, >= total],
        unit column stride, one common row stride) receive columns 0 .. total-1; a field left
        None is not computed.  One kernel on the current stream, nothing allocated besides the
        outputs, so the call can be captured in a HIP graph."""
        iq = _check_iq(iq, self.device)
        F, L = iq.shape
        dev = self.device
        if self.mode == "api":
            self.symbols_per_frame(L)  # the plan's frame-length rule
        total = L // self.step
        cfo, toff, amp = self._frame_offsets(result, F)
        out, m = _metric_outputs(out, F, total, dev)
        stride = iq.stride(0) if F > 1 else L
        _capi.check(self._lib.lora_demod_metrics_batch(self._h, iq.data_ptr(), F, L, stride, cfo, toff, amp,
                                                       C.byref(m), _stream_handle(dev)))
        return out

    def _frame_offsets(self, result: Optional[DemodResult], F: int):
        """(cfo, time_offset, max_amp) device pointers of ``result`` as the plan's mode needs
        them to rebuild each symbol's window; all None for a raw plan."""
        if self.mode == "raw":
            return None, None, None
        if result is None:
            raise ValueError(f"a {self.mode} plan needs result= (the DemodResult of run() on these frames)")
        names = ("cfo", "time_offset") + (("max_amp",) if self.mode == "legacy" else ())
        for name in names:
            _check_buf(getattr(result, name), "result." + name, torch.float32, self.device, F)
        return (result.cfo.data_ptr(), result.time_offset.data_ptr(),
                result.max_amp.data_ptr() if self.mode == "legacy" else None)

    def soft_bits(self, iq: torch.Tensor, result: Optional[DemodResult] = None,
                  out: Optional[torch.Tensor] = None, reduced: Optional[Tuple[int, int]] = None) -> torch.Tensor:
        """Max-log LLRs of the sf bits of every whole symbol (lora_demod_soft_bits_batch) for
        the frames of a [F, L] (or [L]) complex64 CUDA tensor: float32 [F, total, sf], column s
        = symbol s (the sync symbols are columns 0 and 1), positive = the bit of
        grayToBinary16(index) is 1, on the same spectra as ``detect_metrics``.  SF 6-12.

        ``result`` follows ``detect_metrics``' rules (required for legacy / api plans, ignored
        for raw ones).  ``out``: a float32 [>= F, >= total, sf] tensor, contiguous in its last
        two dimensions; the [F, total, sf] view of it that was written is returned.  One kernel
        on the current stream, nothing allocated besides the output, so the call can be captured
        in a HIP graph.

        ``reduced=(first, count)`` (lora_demod_soft_bits_frame_batch, SF 7-12): columns ``first ..
        first + count - 1`` of every frame are symbols of a self-describing frame's header block
        - ``(2, 8)`` after the two sync symbols.  Their first sf - 2 entries are the LLRs of the
        bits of grayToBinary16 of the bin rounded to the nearest multiple of four, the last two
        +0.0; ``codec.decode_frame_soft`` reads them.  ``None`` and ``(first, 0)`` are the plain
        call."""
        iq = _check_iq(iq, self.device)
        F, L = iq.shape
        dev = self.device
        if not 6 <= self.sf <= 12:
            raise ValueError("soft bits need a plan with sf in 6..12")
        red_first, red_count = (0, 0) if reduced is None else (int(reduced[0]), int(reduced[1]))
        if self.mode == "api":
            self.symbols_per_frame(L)  # the plan's frame-length rule
        total = L // self.step
        cfo, toff, amp = self._frame_offsets(result, F)
        if out is None:
            out = torch.empty((F, total, self.sf), dtype=torch.float32, device=dev)
        else:
            _require_cuda(out, "out")
            if out.dtype != torch.float32:
                raise TypeError(f"out must be torch.float32, got {out.dtype}")
            if (out.device != dev or out.dim() != 3 or out.shape[0] < F or out.shape[1] < total
                    or out.shape[2] != self.sf or out.stride(2) != 1
                    or (out.shape[1] > 1 and out.stride(1) != self.sf)
                    or (F > 1 and (out.stride(0) % self.sf or out.stride(0) < total * self.sf))):
                raise ValueError(f"out must be a float32 [>={F}, >={total}, {self.sf}] tensor on {dev}, contiguous "
                                 "in its last two dimensions, with non-overlapping rows")
        llr_stride = out.stride(0) // self.sf if F > 1 else total
        stride = iq.stride(0) if F > 1 else L
        if reduced is None:
            got = _capi.check(self._lib.lora_demod_soft_bits_batch(
                self._h, iq.data_ptr(), F, L, stride, cfo, toff, amp, out.data_ptr() if out.numel() else None,
                llr_stride, _stream_handle(dev)))
        else:
            got = _capi.check(self._lib.lora_demod_soft_bits_frame_batch(
                self._h, iq.data_ptr(), F, L, stride, cfo, toff, amp, out.data_ptr() if out.numel() else None,
                llr_stride, red_first, red_count, _stream_handle(dev)))
        assert got == total, (got, total)
        return out[:F, :total]

    def scan_windows(self, row_len: int, hop: int) -> int:
        """Windows ``scan`` computes per row of ``row_len`` samples: one every ``hop`` samples
        while a whole one (``step``) fits, ``0 if row_len < step else (row_len - step) // hop + 1``
        (lora_detect_scan_windows)."""
        return _capi.check(self._lib.lora_detect_scan_windows(self._h, int(row_len), int(hop)))

    def scan(self, iq: torch.Tensor, hop: int, out: Optional[DetectMetrics] = None) -> DetectMetrics:
        """The sliding detector scan (lora_detect_scan_batch) of continuous streams: a [L] or
        [R, L] complex64 CUDA tensor, one stream per row (rows may be a strided view with
        non-overlapping rows).  Column w of the [R, W] result is the detector on the ``step``
        samples from ``w * hop``, bit-identical to ``detect_metrics`` of a raw plan on those
        samples as one frame: the plan's dechirp and window apply, its mode does not.  Any
        ``hop >= 1``; ``W = scan_windows(L, hop)``.  ``out`` follows ``detect_metrics``' rules
        with W for total.  One kernel on the current stream, nothing allocated besides the
        outputs, so the call can be captured in a HIP graph."""
        iq = _check_iq(iq, self.device)
        R, L = iq.shape
        hop = int(hop)
        if hop < 1:
            raise ValueError("hop must be >= 1")
        W = 0 if L < self.step else (L - self.step) // hop + 1
        out, m = _metric_outputs(out, R, W, self.device)
        stride = iq.stride(0) if R > 1 else L
        got = _capi.check(self._lib.lora_detect_scan_batch(self._h, iq.data_ptr(), R, L, stride, hop, C.byref(m),
                                                           _stream_handle(self.device)))
        assert got == W, (got, W)
        return out

    def scan_acc(self, iq: torch.Tensor, hop: int, acc: int, conj: bool = False,
                 out: Optional[DetectMetrics] = None) -> DetectMetrics:
        """The accumulating scan (lora_detect_scan_acc_batch): ``scan`` with the |X|^2 spectra of
        ``acc`` (1..8) windows one symbol apart summed in fp32, oldest first, before the detector's
        argmax and noise floor - column w of the [R, Wa] result covers the ``acc`` symbols from
        ``w * hop``, ``Wa = max(scan_windows(L, hop) - (acc - 1) * (step // hop), 0)``.  With
        ``acc > 1`` ``hop`` must divide ``step``.  ``conj``: the scan of the conjugated rows, in
        which a down-chirp dechirps as an up-chirp does.  Returns DetectMetrics with ``f_index``
        None (a summed spectrum has no neighbour phases).  ``acc=1`` equals ``scan`` bit for bit.
        ``out`` follows ``scan``'s rules with Wa for W; its ``f_index`` must be None.  One kernel on
        the current stream, nothing allocated besides the outputs; nothing synchronises."""
        iq = _check_iq(iq, self.device)
        R, L = iq.shape
        hop, acc = int(hop), int(acc)
        if hop < 1:
            raise ValueError("hop must be >= 1")
        if not 1 <= acc <= 8:
            raise ValueError("acc must be in 1..8")
        if acc > 1 and self.step % hop:
            raise ValueError(f"with acc > 1, hop must divide step = {self.step} (got {hop})")
        W = 0 if L < self.step else (L - self.step) // hop + 1
        Wa = max(W - (acc - 1) * (self.step // hop), 0) if acc > 1 else W
        dev = self.device
        if out is None:
            out = DetectMetrics(torch.empty((R, Wa), dtype=torch.float32, device=dev),
                                torch.empty((R, Wa), dtype=torch.float32, device=dev), None,
                                torch.empty((R, Wa), dtype=torch.uint16, device=dev))
        elif out.f_index is not None:
            raise ValueError("scan_acc has no f_index: out.f_index must be None")
        out, m = _metric_outputs(out, R, Wa, dev)
        stride = iq.stride(0) if R > 1 else L
        if R and Wa:
            got = _capi.check(self._lib.lora_detect_scan_acc_batch(
                self._h, iq.data_ptr(), R, L, stride, hop, acc, 1 if conj else 0, m.power, m.power_avg, m.index,
                m.stride, _stream_handle(dev)))
            assert got == Wa, (got, Wa)
        return out

    def estimate_offsets(self, iq: torch.Tensor, cfo: torch.Tensor, time_offset: torch.Tensor) -> int:
        """phy.cpp:78-145 over every whole symbol of each frame (raw samples)."""
        iq = _check_iq(iq, self.device)
        F, L = iq.shape
        _check_buf(cfo, "cfo", torch.float32, self.device, F)
        _check_buf(time_offset, "time_offset", torch.float32, self.device, F)
        stride = iq.stride(0) if F > 1 else L
        return _capi.check(self._lib.lora_estimate_offsets_batch(
            self._h, iq.data_ptr(), F, L, stride, cfo.data_ptr(), time_offset.data_ptr(),
            _stream_handle(self.device)))


def compensate_offsets(iq: torch.Tensor, sf: int, osr: int, cfo: torch.Tensor,
                       time_offset: torch.Tensor) -> torch.Tensor:
    """phy.cpp:147-176 for a [F, L] batch; returns a new tensor (out of place)."""
    _require_cuda(iq, "iq")
    squeeze = iq.dim() == 1
    x = _check_iq((iq.unsqueeze(0) if squeeze else iq).contiguous(), iq.device)
    F, L = x.shape
    _check_buf(cfo, "cfo", torch.float32, x.device, F)
    _check_buf(time_offset, "time_offset", torch.float32, x.device, F)
    out = torch.empty_like(x)
    lib = _capi.lib()
    _capi.check(lib.lora_compensate_offsets_batch(
        int(sf), int(osr), x.data_ptr(), F, L, L, cfo.contiguous().data_ptr(),
        time_offset.contiguous().data_ptr(), x.device.index, _stream_handle(x.device),
        out.data_ptr()))
    return out[0] if squeeze else out


class LoRaDemod:
    """Block-style demodulator mirroring the Pothos ``/lora/lora_demod`` surface
    (examples/lora_simulation.pth:427-445: sf, sync, thresh, mtu) plus the library
    parameters bw / cr / osr / window (phy.hpp:51-58).

    ``work(iq)`` consumes one frame (or a [F, L] batch) of raw IQ and returns the
    symbol stream; per-frame metrics of the last call are in ``last``.

    The Pothos-only parameters (the upstream block is an empty submodule in the
    reference, so their semantics are not pinned by any reference code):
      * ``mtu`` - the most data symbols one frame (packet) yields: ``work`` returns at
        most ``mtu`` symbols per frame (the first ones); ``last`` keeps them all.
      * ``thresh`` - a detection threshold in dB.  The reference library path
        (LoRaDemod.cpp:49-195) has no detection gate, so no gate is applied; only the
        graph's value -30.0 (examples/lora_simulation.pth:440) is accepted, and any
        other value raises instead of being silently ignored.  The values such a gate would
        compare - the detector's per-symbol power and noise floor - come from
        ``work_metrics``; what to do with them is the caller's decision.
    """

    THRESH_DEFAULT = -30.0

    def __init__(self, sf: int, sync: int = 0x12, thresh: float = -30.0, mtu: int = 256,
                 bw: int = 125000, cr: int = 1, osr: int = 1, window="none",
                 dechirp: bool = True, mode: str = "legacy", device=None, precision: str = "exact"):
        if float(thresh) != self.THRESH_DEFAULT:
            raise ValueError(f"thresh={thresh}: no detection gate is defined by the reference path; "
                             f"only the default {self.THRESH_DEFAULT} is accepted")
        if int(mtu) < 1:
            raise ValueError("mtu must be >= 1 symbol")
        self.sf, self.sync, self.thresh, self.mtu = int(sf), int(sync) & 0xFF, float(thresh), int(mtu)
        self.bw, self.cr, self.osr = int(bw), int(cr), int(osr) if osr else 1
        self.plan = DemodPlan(sf, self.osr, bw, window, dechirp, mode, device, precision)
        self.last: Optional[DemodResult] = None

    def work(self, iq: torch.Tensor) -> torch.Tensor:
        res = self.plan.run(iq)
        self.last = res
        syms = res.symbols[:, :self.mtu]
        return syms[0] if iq.dim() == 1 else syms

    def work_frames(self, iq: torch.Tensor) -> DemodResult:
        self.last = self.plan.run(iq)
        return self.last

    def work_payload(self, iq: torch.Tensor, nbytes: Optional[int] = None, chain: str = "library"):
        """Demodulate, then decode the symbols on the device (lora_phy_amd.codec): payload
        bytes come out and nothing visits the host.  Returns a codec.DecodeResult; the
        demodulator's own per-frame results are in ``last``.

        ``chain="library"``: lora_decode with the CRC check of lora_phy::decode
        (phy.cpp:241-256) over the first ``2 * nbytes`` symbols of each frame (default: all
        of them).  ``chain="lora"``: the coding chain at this block's ``sf`` and ``cr``
        (Gray, deinterleave, de-whitening, nibble decode) to ``nbytes`` bytes (default: as
        many as the frame's whole blocks carry, at most 255)."""
        from . import codec

        if chain not in ("library", "lora"):
            raise ValueError('chain must be "library" or "lora"')
        self.last = self.plan.run(iq)
        syms = self.last.symbols
        if iq.dim() == 1:
            syms = syms[0]
        if chain == "lora":
            if nbytes is None:
                nbytes = codec.chain_capacity(self.sf, self.cr, syms.shape[-1])
            return codec.decode_chain(syms, self.sf, self.cr, nbytes)
        if nbytes is not None:
            if not 0 <= 2 * int(nbytes) <= syms.shape[-1]:
                raise ValueError(f"nbytes={nbytes} needs {2 * int(nbytes)} symbols, the frames have {syms.shape[-1]}")
            syms = syms[..., :2 * int(nbytes)]
        return codec.decode(syms)

    def work_payload_soft(self, iq: torch.Tensor, nbytes: Optional[int] = None):
        """``work_payload(..., chain="lora")`` with soft decisions: demodulate (``last`` is set
        as by ``work_payload``), take the per-bit LLRs of the same frames
        (``DemodPlan.soft_bits``) and decode their data columns through the chain at this
        block's ``sf`` and ``cr`` by maximum likelihood (``codec.decode_chain_soft``) to
        ``nbytes`` bytes (default: as many as the frame's whole blocks carry, at most 255).
        Returns a codec.DecodeResult whose ``errors`` counts the codewords the soft decision
        changed.  The sync word in ``last`` stays a hard decision."""
        from . import codec

        self.last = self.plan.run(iq)
        llr = self.plan.soft_bits(iq, self.last)
        if self.plan.mode != "raw":
            llr = llr[:, 2:]  # the sync symbols' columns
        if nbytes is None:
            nbytes = codec.chain_capacity(self.sf, self.cr, llr.shape[1])
        return codec.decode_chain_soft(llr[0] if iq.dim() == 1 else llr, self.sf, self.cr, nbytes)

    def work_metrics(self, iq: torch.Tensor) -> DetectMetrics:
        """Demodulate (``last`` is set as by ``work_frames``), then return the detector's
        per-symbol power, noise floor and fractional index for the same frames
        (``DemodPlan.detect_metrics``): the link quality behind ``last.symbols``.  No gate
        acts on them (see ``thresh``)."""
        self.last = self.plan.run(iq)
        return self.plan.detect_metrics(iq, self.last)

    def work_stream(self, iq: torch.Tensor, frame_symbols: int, hop: Optional[int] = None,
                    thresh_db: float = 0.0):
        """Receive a continuous [L] stream (``lora_phy_amd.stream.receive`` with this block's plan
        and sync word): scan, find the frames of ``frame_symbols`` data symbols, cut them out and
        demodulate them.  Returns ``(starts, symbols[:, :mtu])`` - the int64 [K] sample index of
        each frame's first sync symbol and its data symbols; ``last`` keeps the DemodResult of
        the K frames.  ``thresh_db`` gates ``power - power_avg`` of both sync windows and has
        nothing to do with ``thresh``, which stays as it is."""
        from . import stream

        starts, res = stream.receive(self.plan, iq, frame_symbols, hop, self.sync, thresh_db)
        self.last = res
        return starts, res.symbols[:, :self.mtu]

    def work_wideband(self, chan, iq: torch.Tensor, frame_symbols: int, hop: Optional[int] = None,
                      thresh_db: float = 0.0, scale: Optional[float] = None):
        """``work_stream`` for a wideband capture (``lora_phy_amd.stream.receive_wideband`` with
        this block's plan and sync word): ``chan``, a ``stream.Channelizer``, turns the [L] stream
        (complex64, or raw [L, 2] integer samples converted with ``scale``) into its channel rows, whose frames are found and demodulated.  Returns ``(channel,
        starts, symbols[:, :mtu])`` - per frame its channel and the sample index, in channel
        samples, of its first sync symbol, ordered by channel then start; ``last`` keeps the
        DemodResult of the K frames.  Frame i began near wideband sample ``starts[i] * chan.decim /
        chan.interp + chan.delay``.  This block's ``osr`` and bw must be the channel rows': the
        wideband rate must be ``bw * osr * chan.decim / chan.interp``."""
        from . import stream

        channel, starts, res = stream.receive_wideband(self.plan, chan, iq, frame_symbols, hop, self.sync,
                                                       thresh_db, scale)
        self.last = res
        return channel, starts, res.symbols[:, :self.mtu]

    def work_stream_device(self, iq: torch.Tensor, frame_symbols: int, hop: Optional[int] = None,
                           thresh_db: float = 0.0, first=None, capacity: Optional[int] = None):
        """``work_stream`` without the host (``lora_phy_amd.stream.receive_device`` with this block's
        plan and sync word): a [L] stream or [R, L] rows.  Returns ``(found, symbols[:, :, :mtu])``
        - the stream.FoundFrames (count [R], starts [R, capacity], end [R]) and the data symbols of
        every slot, [R, capacity, <= mtu]; only the slots of ``found.valid`` hold a frame.  ``last``
        keeps the DemodResult of all ``R * capacity`` slots.  Nothing synchronises."""
        from . import stream

        got = stream.receive_device(self.plan, iq, frame_symbols, hop, self.sync, thresh_db, first, capacity)
        self.last = got.result
        R, cap = got.found.starts.shape
        return got.found, got.result.symbols.reshape(R, cap, got.result.symbols.shape[1])[:, :, :self.mtu]

    def work_wideband_device(self, chan, iq: torch.Tensor, frame_symbols: int, hop: Optional[int] = None,
                             thresh_db: float = 0.0, scale: Optional[float] = None, first=None,
                             capacity: Optional[int] = None):
        """``work_wideband`` without the host (``lora_phy_amd.stream.receive_wideband_device`` with
        this block's plan and sync word).  Returns ``(found, symbols[:, :, :mtu])`` as
        ``work_stream_device`` does, row r being channel r and starts in channel samples; ``last``
        keeps the DemodResult of all ``C * capacity`` slots.  Nothing synchronises."""
        from . import stream

        got = stream.receive_wideband_device(self.plan, chan, iq, frame_symbols, hop, self.sync, thresh_db, scale,
                                             first, capacity)
        self.last = got.result
        R, cap = got.found.starts.shape
        return got.found, got.result.symbols.reshape(R, cap, got.result.symbols.shape[1])[:, :, :self.mtu]

    def work_packets_device(self, iq: torch.Tensor, max_symbols: Optional[int] = None, hop: Optional[int] = None,
                            thresh_db: float = 0.0, first=None, capacity: Optional[int] = None,
                            cand_capacity: Optional[int] = None, soft: bool = False, max_flips: int = 5):
        """Receive self-describing frames (``LoRaMod.work_frame``) from a [L] stream or [R, L] rows
        with no frame length given (``lora_phy_amd.stream.receive_frames_device`` with this block's
        plan and sync word): each frame's header states its length, coding rate and CRC flag, and
        the header's coding rate wins over this block's ``cr``.  ``max_symbols``: the longest frame
        accepted, by default ``mtu``.  Returns the stream.StreamPackets - ``found``, ``nsym``, and
        ``frames`` with every slot's status and payload; select with ``found.valid``.  ``last``
        keeps the DemodResult of all slots.  ``soft`` and ``max_flips``: the header probe and the
        decode on soft bits, as ``receive_frames_device``'s.  Nothing synchronises."""
        from . import stream

        got = stream.receive_frames_device(self.plan, iq, self.mtu if max_symbols is None else max_symbols, hop,
                                           self.sync, thresh_db, first, capacity, cand_capacity, soft=soft,
                                           max_flips=max_flips)
        self.last = got.result
        return got

    def work_wideband_packets_device(self, chan, iq: torch.Tensor, max_symbols: Optional[int] = None,
                                     hop: Optional[int] = None, thresh_db: float = 0.0,
                                     scale: Optional[float] = None, first=None, capacity: Optional[int] = None,
                                     cand_capacity: Optional[int] = None):
        """``work_packets_device`` for a wideband capture
        (``lora_phy_amd.stream.receive_wideband_frames_device``): row r of the result is channel r
        of ``chan``, starts are in channel samples.  Nothing synchronises."""
        from . import stream

        got = stream.receive_wideband_frames_device(self.plan, chan, iq, self.mtu if max_symbols is None
                                                    else max_symbols, hop, self.sync, thresh_db, scale, first,
                                                    capacity, cand_capacity)
        self.last = got.result
        return got

    def work_preamble_device(self, iq: torch.Tensor, max_symbols: Optional[int] = None, preamble_acc: int = 6,
                             hop: Optional[int] = None, thresh_up_db: Optional[float] = None,
                             thresh_dn_db: Optional[float] = None, max_cfo_bins: Optional[int] = None, first=None, capacity: Optional[int] = None,
                             cand_capacity: Optional[int] = None, soft: bool = False, max_flips: int = 5):
        """``work_packets_device`` for preambled frames (``LoRaMod.work_frame(preamble=...)``) under a
        carrier offset of whole bins (``lora_phy_amd.stream.receive_preamble_frames_device`` with this
        block's plan): the StreamPackets also hold each frame's ``cfo_bins``.  Nothing
        synchronises."""
        from . import stream

        got = stream.receive_preamble_frames_device(self.plan, iq, self.mtu if max_symbols is None else max_symbols,
                                                    preamble_acc, hop, self.sync, thresh_up_db, thresh_dn_db,
                                                    max_cfo_bins, first, capacity, cand_capacity, soft=soft,
                                                    max_flips=max_flips)
        self.last = got.result
        return got

    def sync_ok(self) -> torch.Tensor:
        """Per-frame flag: recovered sync word equals the configured one."""
        if self.last is None:
            raise RuntimeError("work() has not run")
        return self.last.sync == self.sync


_PIPELINE = threading.local()


@contextlib.contextmanager
def spec_pipeline(enabled: bool = True):
    """Plans created inside this block ON THIS THREAD use the speculative single-read pipeline
    (``enabled=True``, whatever LORA_MI355X_SPEC says) or the three-launch exact path (frame
    max, estimate, demod: ``enabled=False``) - ``DemodPlan(pipeline=...)`` with the choice
    filled in.  Nothing process-wide changes (no environment variable is touched), so other
    threads creating plans meanwhile are unaffected; blocks nest."""
    prev = getattr(_PIPELINE, "choice", None)
    _PIPELINE.choice = "spec" if enabled else "split"
    try:
        yield
    finally:
        _PIPELINE.choice = prev
