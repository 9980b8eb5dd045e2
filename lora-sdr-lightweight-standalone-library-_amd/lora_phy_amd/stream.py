"""Stream receive: find the frames of a continuous recording and demodulate them.

Every other entry point takes frames that are already cut, each row starting on its first
sync symbol.  Here the start is found: ``DemodPlan.scan`` runs the reference's detector
(LoRaDetector.hpp:39-74) on a window every ``hop`` samples, ``find_frames`` turns its outputs
into frame starts, ``extract_frames`` gathers the frames and the plan's ``run`` demodulates
them as always; ``receive`` is the four in a row.

The reference has no frame detector (its only preamble handling is the estimate over the two
sync symbols of a frame that is already aligned), so the finder's rule is this project's own.
It is defined on the detector's outputs alone:

* The scan is made by a plan with ``dechirp=True`` at bw 125 kHz, SF 6-12, with ``hop`` dividing
  ``step = N * osr`` and ``k = step // hop >= 2``.  (At other bandwidths a timing shift moves
  the bin by bw_scale per sample and the refinement below is ambiguous.)
* ``N = 2**sf``, ``sw0 = (sync >> 4) << (sf - 4)``, ``sw1 = (sync & 15) << (sf - 4)``: the two sync
  symbols; ``frame_len = (frame_symbols + 2) * step``.
* ``snr[w] = power[w] - power_avg[w]`` (an fp32 subtraction; NaN fails every comparison).
* Window w, ``0 <= w < W - k``, is a candidate when ``snr[w] >= thresh_db``, ``snr[w + k] >=
  thresh_db`` and ``(index[w + k] - index[w]) mod N == (sw1 - sw0) mod N``: two windows one
  symbol apart whose peaks differ as the sync symbols do.
* Refinement: a window that starts d chips into a symbol sees that symbol's bin raised by d, so
  ``d = (index[w] - sw0) mod N`` (minus N when ``d >= N / 2``) and ``start = w * hop - d * osr``.
* Greedy pass in increasing w from ``ceil(max(first - step / 2, 0) / hop)``: a candidate with
  ``start >= first`` and ``start + frame_len <= row_len`` is accepted, ``first`` becomes
  ``start + frame_len`` and the pass continues at the smallest ``w' > w`` with
  ``w' * hop >= first - step / 2``; anything else moves on to ``w + 1``.

Limits.  The resolution is ``osr`` samples: the demodulator's own osr-phase estimate takes it
from there.  A stream that begins inside a frame can produce a false start, with probability
of about 1/N per pair of consecutive symbols; a sync word with equal nibbles makes any repeated
symbol a candidate.  No detection-probability figure is claimed, because none has been
measured.  A perfectly aligned noiseless window has no noise floor (``power_avg = -inf``, so
``snr = +inf`` and it passes any threshold); a silent window gives NaN and never passes.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from .demod import DemodPlan, DemodResult, DetectMetrics, _check_iq

__all__ = ["find_frames", "extract_frames", "receive"]

_NONE = -(1 << 62)  # "no candidate here" in the packed starts


def _geometry(hop: int, sf: int, osr: int, frame_symbols: int, sync: int, bw: int):
    sf, osr, hop = int(sf), int(osr) if osr else 1, int(hop)
    if int(bw) != 125000:
        raise ValueError("the frame finder is defined at bw 125000 only")
    if not 6 <= sf <= 12:
        raise ValueError("the frame finder needs SF 6-12")
    if int(frame_symbols) < 0:
        raise ValueError("frame_symbols must be >= 0")
    N = 1 << sf
    step = N * osr
    if hop < 1 or step % hop != 0 or step // hop < 2:
        raise ValueError(f"hop must divide step = {step} at least twice (got {hop})")
    sync = int(sync) & 0xFF
    sw0, sw1 = (sync >> 4) << (sf - 4), (sync & 15) << (sf - 4)
    return N, step, step // hop, sw0, sw1, (int(frame_symbols) + 2) * step


def _ceil_div(a: int, b: int) -> int:
    return -((-a) // b)


def _find(metrics: DetectMetrics, hop, sf, osr, frame_symbols, sync, thresh_db, first, row_len, bw) -> np.ndarray:
    N, step, k, sw0, sw1, frame_len = _geometry(hop, sf, osr, frame_symbols, sync, bw)
    hop, osr = int(hop), step // N
    power, floor, index = (t.reshape(-1) if t.dim() == 2 and t.shape[0] == 1 else t
                           for t in (metrics.power, metrics.power_avg, metrics.index))
    if power.dim() != 1 or floor.shape != power.shape or index.shape != power.shape:
        raise ValueError("find_frames takes the metrics of one row: power, power_avg and index of one [W] shape")
    W = power.shape[0]
    if row_len is None:
        row_len = (W - 1) * hop + step if W else 0
    if W <= k:
        return np.zeros(0, np.int64)
    # the candidate mask and each candidate's refined start, on the tensors' device
    ok = (power - floor) >= float(thresh_db)
    idx = index.to(torch.int64)
    n = W - k
    cand = ok[:n] & ok[k:] & (torch.remainder(idx[k:] - idx[:n], N) == (sw1 - sw0) % N)
    d = torch.remainder(idx[:n] - sw0, N)
    d = torch.where(d >= N // 2, d - N, d)
    start = torch.arange(n, dtype=torch.int64, device=power.device) * hop - d * osr
    packed = torch.where(cand, start, torch.full_like(start, _NONE)).cpu().numpy()  # the one synchronisation
    # the greedy pass, on the host, over the candidates only
    first = int(first)
    wmin = _ceil_div(max(first - step // 2, 0), hop)
    out = []
    for w in np.flatnonzero(packed != _NONE):
        w, s = int(w), int(packed[w])
        if w < wmin or s < first or s + frame_len > row_len:
            continue
        out.append(s)
        first = s + frame_len
        wmin = max(w + 1, _ceil_div(max(first - step // 2, 0), hop))
    return np.array(out, np.int64)


def find_frames(metrics: DetectMetrics, hop: int, sf: int, osr: int, frame_symbols: int, sync: int = 0x12,
                thresh_db: float = 0.0, first: int = 0, row_len: Optional[int] = None,
                bw: int = 125000) -> torch.Tensor:
    """Frame starts in one scanned row, by the rule in this module's docstring: an int64 [K]
    tensor, increasing, on the metrics' device.

    ``metrics``: ``DemodPlan.scan``'s result for one row ([W] or [1, W] tensors; power,
    power_avg and index are used), made with this ``hop`` by a dechirping plan of this ``sf``
    and ``osr``.  Frames have ``frame_symbols`` data symbols after the two sync symbols.
    ``first``: no frame starts before this sample (where the last accepted frame ended, when a
    long recording is received in chunks).  ``row_len``: the row's length in samples, which a
    frame must fit in (default: the span the W windows cover, ``(W - 1) * hop + step``).

    Plain tensor operations, so CPU tensors work as well.  The candidate mask and the refined
    starts are computed on the tensors' device; the greedy pass runs on the host over the
    candidates only, after one copy to the host: one synchronisation per call.
    ``ValueError``: bw other than 125000, SF outside 6-12, ``hop`` not dividing ``step`` or
    ``step // hop < 2``."""
    got = _find(metrics, hop, sf, osr, frame_symbols, sync, thresh_db, first, row_len, bw)
    return torch.from_numpy(got).to(metrics.power.device)


def _gather(iq: torch.Tensor, starts: torch.Tensor, frame_len: int) -> torch.Tensor:
    windows = iq.as_strided((iq.shape[0] - frame_len + 1, frame_len), (iq.stride(0), iq.stride(0)))
    return windows.index_select(0, starts)


def extract_frames(iq: torch.Tensor, starts: torch.Tensor, frame_len: int) -> torch.Tensor:
    """``iq[s : s + frame_len]`` for every s of ``starts`` as a new [K, frame_len] tensor on
    ``iq``'s device: one gather, no host loop.  ``iq`` is a 1-D stream, ``starts`` an integer
    [K] tensor; every frame must lie inside the stream (checked, which costs one
    synchronisation when the tensors are on the device)."""
    frame_len = int(frame_len)
    if iq.dim() != 1 or starts.dim() != 1 or frame_len < 0:
        raise ValueError("extract_frames takes a 1-D stream, a 1-D tensor of starts and frame_len >= 0")
    starts = starts.to(device=iq.device, dtype=torch.int64)
    if starts.numel() == 0:
        return iq.new_empty((0, frame_len))
    lo, hi = (int(v) for v in torch.stack(torch.aminmax(starts)).cpu())
    if lo < 0 or hi + frame_len > iq.shape[0]:
        raise ValueError(f"frames of {frame_len} samples at {lo}..{hi} leave the stream of {iq.shape[0]} samples")
    return _gather(iq, starts, frame_len)


def receive(plan: DemodPlan, iq: torch.Tensor, frame_symbols: int, hop: Optional[int] = None, sync: int = 0x12,
            thresh_db: float = 0.0) -> Tuple[torch.Tensor, DemodResult]:
    """Scan, find, extract, demodulate: the frames of ``frame_symbols`` data symbols in the
    continuous stream ``iq`` (a [L] complex64 CUDA tensor on the plan's device).

    Returns ``(starts, result)``: the int64 [K] sample index of each frame's first sync symbol
    and ``plan.run``'s DemodResult for the K frames cut there.  ``hop`` defaults to
    ``step // 4``.  The plan must dechirp (``dechirp=True``) at bw 125 kHz; its mode and window
    are the demodulator's to choose.  With no frame found the tensors are empty and no demod
    call is made.  One synchronisation (``find_frames``)."""
    if not plan.dechirp:
        raise ValueError("receive needs a plan with dechirp=True: the finder reads dechirped peaks")
    if iq.dim() != 1:
        raise ValueError("receive takes one [L] stream")
    iq = _check_iq(iq, plan.device)[0]
    hop = plan.step // 4 if hop is None else int(hop)
    geo = _geometry(hop, plan.sf, plan.osr, frame_symbols, sync, plan.bw)
    frame_len = geo[-1]
    met = plan.scan(iq, hop)
    starts = _find(met, hop, plan.sf, plan.osr, frame_symbols, sync, thresh_db, 0, iq.shape[0], plan.bw)
    dev = plan.device
    K = len(starts)
    starts_t = torch.from_numpy(starts).to(dev)
    if K == 0:
        return starts_t, DemodResult(symbols=torch.empty((0, int(frame_symbols)), dtype=torch.uint16, device=dev),
                                     sync=torch.empty(0, dtype=torch.uint8, device=dev),
                                     cfo=torch.empty(0, dtype=torch.float32, device=dev),
                                     time_offset=torch.empty(0, dtype=torch.float32, device=dev),
                                     max_amp=torch.empty(0, dtype=torch.float32, device=dev))
    # (the finder only accepts frames that fit the stream, so the gather needs no second check)
    return starts_t, plan.run(_gather(iq, starts_t, frame_len))

