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
symbol a candidate.  Detection probability, measured once (profiles/stream/detect_prob.json,
``tools/detect_prob.py``: osr 1, frames of 16 symbols at unit amplitude under ``impair``'s noise,
``hop = step / 4``, ``thresh_db = 0``, 2,000 frames per point, a detection being a planted start
returned exactly): the finder's edge lies between 0 and +5 dB at every SF - SF7 0.06 / 0.66 / 0.995
at 0 / +2 / +4 dB, SF12 0.007 / 0.77 / 1.0 at 0 / +2 / +3 dB, nothing at or below -2 dB - because
``power - power_avg`` is the peak bin over the sum of all the others, which follows the SNR per
sample: with the default threshold the finder does not use the spreading gain, though every
detected frame demodulated with all its symbols right.  A carrier offset of a quarter bin costs
about 2 dB more (SF7 0.82, SF12 0.95 at +5 dB): it moves the refinement's peak between bins.
Noise alone gave no false start in 10^7 windows per SF; with frames present up to 150 returned
starts per 10^6 windows were not the planted ones (SF7, +1 dB).  Other thresholds, osr > 1 and
integer-bin offsets have not been measured.  A perfectly aligned noiseless window has no noise floor (``power_avg = -inf``, so
``snr = +inf`` and it passes any threshold); a silent window gives NaN and never passes.

The finder on the device.  ``find_frames`` computes the candidates on the device, copies every
window's packed start to the host and runs the greedy pass there: one synchronisation per call,
the only one of ``receive``.  ``find_frames_device`` is the same rule as one kernel
(lora_find_frames_batch, csrc/lora_find.hip): the accepted starts of every row stay on the
device, in a fixed number of slots per row with a count beside them (``FoundFrames``), and
``receive_device`` / ``receive_wideband_device`` demodulate all the slots without ever reading
device memory on the host - so the next chunk can be enqueued before anyone looks at this one's
count.  The outputs equal the host finder's as integers.

Frames that state their own length.  Everything above takes ``frame_symbols`` from its caller,
so one call receives one kind of traffic.  ``receive_frames_device`` receives self-describing
frames (``codec.encode_frame``: an explicit header with the payload length, the coding rate and
a CRC flag under a 5-bit checksum, in a first block of eight symbols) of any mix of lengths and
coding rates, and is given only ``max_symbols``, the longest frame it should accept.  The
candidate rule and refinement above are unchanged; what changes is what happens to a candidate:

* ``find_candidates_device`` lists, per row and in increasing w, each candidate's ``start`` with
  ``start >= 0`` and ``start + 10 * step <= row_len``, unless it equals the row's last listed one
  (``cand_capacity`` slots per row, ``ceil(row_len / (4 * step))`` by default, a count beside them);
* ``gather_frames_device`` cuts ``10 * step`` samples at each, ``plan.run`` demodulates them and
  ``codec.decode_header`` decodes the eight symbols: a status and, when the header is good, the
  frame's ``nsym``;
* ``select_frames_device`` is the greedy pass over the slots, in slot order: slot j is accepted
  when its status is OK, ``nsym <= max_symbols``, ``start >= first`` and ``start + (2 + nsym) * step
  <= row_len``, and ``first`` becomes that end.  (The fixed-length rule's jump to ``first - step /
  2`` is implied: ``|d * osr| <= step / 2``.)  The result is a ``FoundFrames`` plus each frame's
  ``nsym``;
* a second gather cuts ``(2 + max_symbols) * step`` samples per slot, of which ``(2 + nsym) *
  step`` are the frame's and the rest zeros, so a slot's demodulation is a function of its frame
  alone; ``plan.run``; ``codec.decode_frame`` with ``avail = nsym``.

Of 20,000 random 8-symbol headers per SF, 2 to 5 pass the header's checks, so the header is also
the guard against false candidates that a negative ``thresh_db`` admits - the experiment the
measurement above left open; DESIGN.md §6n has what was measured.  Limits: bw 125 kHz and the
``hop`` rules as above, SF 7-12 (the header block carries ``sf - 7`` data nibbles), hard decisions
only, no implicit-header mode, and no claim of decoding a real LoRa radio.  (``soft=True`` decides
on soft bits; frames with a preamble and a delimiter are the next paragraph's.)
The host model of the chain lives in tests/frame_checker.py.

Preambled frames under a carrier offset.  The finder above decides on two single windows and
cannot tell an offset of whole bins from a timing shift: every start it returns moves by that many
chips.  ``LoRaMod.work_frame(preamble=P)`` / ``modulate_preamble`` put ``P`` plain up-chirps in front
of the two sync symbols and two and a quarter down-chirps (``tail = 9 * step // 4`` samples) between
them and the data - the layout is this project's own, stated to the bit in include/lora_mi355x.h;
each part starts at phase 0, so ``[sync | data]`` gathered from a preambled frame is the plain
frame bit for bit - and ``receive_preamble_frames_device`` finds them from summed spectra:

* ``up = plan.scan_acc(rows, hop, m)`` and ``dn = plan.scan_acc(rows, hop, 2, conj=True)``: the scan
  with the |X|^2 spectra of ``m`` (``preamble_acc``, 2..8) and of 2 windows one symbol apart summed
  in fp32 before the detector's argmax and floor; in the conjugated stream a down-chirp dechirps as
  an up-chirp does.  ``k = step // hop >= 4``, SF 7-12, bw 125 kHz.
* A window ``d`` chips late under an offset of ``c`` bins sees bin ``d + c`` on the up side and ``d -
  c`` on the down side.  For down window ``w`` with ``(2 + m) * k <= w``, ``w + k < Wd`` and ``u = w -
  (2 + m) * k < Wu``, all of: (1) ``dn.power[w] - dn.power_avg[w] >= thresh_dn_db`` and
  ``up.power[u] - up.power_avg[u] >= thresh_up_db`` in fp32 (NaN fails, +inf passes); (2)
  ``dn.power[w] >= dn.power[w - k]`` and ``dn.power[w] > dn.power[w + k]``: the symbol where both
  summed windows lie on down-chirps; (3) ``s = (up.index[u] + dn.index[w]) mod N`` centred to
  ``[-N/2, N/2)``, ``d = floor(s / 2)``, ``c = (up.index[u] - d) mod N`` centred, and ``|c| <=
  max_cfo_bins`` (0 .. N/4 - 1), which rejects the ``(d +- N/2, c +- N/2)`` alias that windows near a
  quarter symbol off produce; (4) ``start = w * hop - d * osr - 2 * step``, the first sync symbol,
  with ``start >= 0`` and ``start + 10 * step + tail <= row_len``.
* A candidate is listed in increasing ``w`` unless its ``(start, c)`` equals that of the previous
  window that passed 1-4 (``find_preamble_device``).  Each is probed as above - gathered as
  ``[sync | data]``, the delimiter skipped, and derotated by ``impair`` with the word ``floor(-c *
  2**32 / step)`` (phase 0 at the slot's first sample, so the phase steps at the join, which a
  demodulator that is non-coherent across symbols does not see) - and ``select_preamble_device``
  runs the greedy pass with ``tail`` added to every frame's length, carrying ``c`` to the accepted
  slot (``StreamPackets.cfo_bins``).

Limits: integer bins only - the residual fraction stays with the demodulator's own estimate - no
fractional delay or drift, ``preamble_acc <= P``, offsets up to ``N / 4 - 1`` bins, and the finder
kernels take one workgroup per row (as ``find_candidates_device``).  The accumulating kernel
recomputes the ``acc`` spectra of every output window (``acc`` times the plain scan's work); a form
that transforms each window once is not built.  Measured once (profiles/stream/preamble_prob.json,
``tools/preamble_prob.py``, DESIGN.md 6p: 600 frames per point, offsets 0 and 3.25 bins): under the
offset the chain above returns no planted frame at any SNR and this one reports 3 bins on every
frame it returns; the edge moves by at least 6 dB at SF12 (every frame at -20 dB), about 2 dB at
SF9 and not at SF7, where header and payload fail with the finder; and at thresholds as low as
noise alone allows (-16 / -22 / -28 dB) a frame's own data symbols list about 18 candidates and
crowd the default candidate capacity, so the chain's thresholds default to 6 dB above those
(``preamble_threshold_db``).  The host model lives in tests/preamble_checker.py.

Wideband captures.  An SDR delivers one wideband stream that holds several LoRa channels at
known offsets from the tuner frequency.  ``Channelizer`` is the stage in front of the scan: one
kernel mixes every channel down, low-pass filters and decimates it (lora_channelize_batch; the
exact arithmetic is in include/lora_mi355x.h and, like the finder's rule, is this project's own:
the reference has no channelizer), and ``receive_wideband`` is ``receive`` over all the channel
rows at once.  Channel centres are multiples of ``fs / period``; the input rate must be
``bw * osr * decim / interp`` - an integer ``decim`` alone, or with ``interp > 1`` the rational
bank (lora_resample_channelize_batch), whose ratios are those with ``interp <= 16`` and ``decim <=
256`` (2.4 MS/s to 125 kS/s is 5/96; 2.048 MS/s, 125/2048, is beyond them); the finder's 125 kHz
restriction is inherited; and the detection probability above was measured on narrowband rows,
not through a bank.

Raw SDR samples.  No radio delivers complex64: an RTL-SDR writes unsigned 8-bit pairs (cu8), a
HackRF signed 8-bit pairs (cs8), USRP, Pluto, LimeSDR and most ``.sigmf-data`` files signed 16-bit
pairs (cs16).  Torch has no complex integers, so a raw capture is an integer tensor with a
trailing dimension of 2 - ``[L, 2]`` for a stream, ``[R, L, 2]`` for rows, dtype ``int16``,
``int8`` or ``uint8`` - and the format follows from the dtype.  A stored component ``v`` stands for
``x = (float(v) - bias) * scale`` in fp32, one rounding per operation, with ``bias = 127.5`` for
``uint8`` and none for the signed dtypes; ``raw_scale(dtype)`` is the default ``scale`` (1/32768,
1/128, 1/127.5, rounded to fp32).  ``Channelizer.run``, ``receive_wideband`` and
``LoRaDemod.work_wideband`` take such a tensor as it is: the bank's kernel converts while it
loads (lora_channelize_raw_batch, lora_resample_channelize_raw_batch), so the integer bytes are
the only read of the capture and no complex64 copy of it ever exists.  ``raw_to_complex`` is the
same conversion in torch operations, for a narrowband user to put in front of ``receive``; the two
agree bit for bit.  ``lora_phy_amd.iq_io`` reads, writes and makes raw captures (``read_raw``,
``iter_stream_raw``, ``write_raw``, ``quantize``).  Nothing here corrects what an SDR front end
does to the samples - DC offset, IQ imbalance, gain steps: the conversion is the whole of it.

Wideband transmit.  ``Synthesizer`` is the inverse of ``Channelizer``: one kernel scales every
channel stream by its gain, interpolates it by an integer ``interp``, mixes it up to its centre
and sums the channels into the one wideband stream a radio transmits, as complex64 or as the raw
integer samples the radio takes (lora_synthesize_batch, lora_synthesize_raw_batch; the exact
arithmetic is in include/lora_mi355x.h and is this project's own: the reference has no
synthesiser).  ``transmit_wideband`` places modulated frames in their channels and runs it, and
``LoRaMod.work_wideband`` modulates first.  Rational up-rates are not covered, and no
spectral-mask or adjacent-channel figure is claimed.

The channel.  Between a transmitter and a receiver stand ``propagate`` - up to eight paths, each a
fractional delay through a table of 256 interpolating filters (``fracdelay_table``) times a complex
gain, a sample-clock offset that slides the reading position and a carrier offset that may drift
(lora_propagate_batch) - and then ``impair``: a gain, a carrier offset, counter-based white noise
and, given a raw dtype, the quantiser (lora_impair_batch, lora_impair_raw_batch).  Both are one
kernel each, defined to the bit in include/lora_mi355x.h as this project's own, reproducible in
chunks, and restated in numpy (tests/propagate_checker.py, tests/impair_checker.py).  The
composition is ``transmit_wideband`` -> ``propagate`` -> ``impair`` -> ``receive_*``.  Fading
(time-varying gains) and front-end effects are not covered.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple, Union

import numpy as np
import torch

from . import _capi
from .demod import DemodPlan, DemodResult, DetectMetrics, _check_iq, _require_cuda, _stream_handle

__all__ = ["find_frames", "extract_frames", "receive", "lowpass_taps", "nco_table", "Channelizer",
           "receive_wideband", "raw_scale", "raw_to_complex", "Synthesizer", "transmit_wideband",
           "FoundFrames", "StreamFrames", "find_frames_device", "receive_device", "receive_wideband_device",
           "impair", "cfo_word", "noise_sigma", "gather_frames_device", "StreamPackets", "find_candidates_device",
           "select_frames_device", "receive_frames_device", "receive_wideband_frames_device",
           "preamble_threshold_db", "find_preamble_device", "select_preamble_device", "receive_preamble_frames_device",
           "receive_wideband_preamble_frames_device", "propagate", "fracdelay_table", "delay_word", "sfo_word",
           "cfo_word64", "drift_word"]

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


def _candidates(power, floor, index, hop, N, osr, k, sw0, sw1, thresh_db) -> torch.Tensor:
    """The candidate mask and each candidate's refined start along the last dimension ([W] or
    [R, W] tensors), on the tensors' device: int64 [.., W - k], ``_NONE`` where no candidate."""
    n = power.shape[-1] - k
    ok = (power - floor) >= float(thresh_db)
    idx = index.to(torch.int64)
    cand = ok[..., :n] & ok[..., k:] & (torch.remainder(idx[..., k:] - idx[..., :n], N) == (sw1 - sw0) % N)
    d = torch.remainder(idx[..., :n] - sw0, N)
    d = torch.where(d >= N // 2, d - N, d)
    start = torch.arange(n, dtype=torch.int64, device=power.device) * hop - d * osr
    return torch.where(cand, start, torch.full_like(start, _NONE))


def _greedy(packed: np.ndarray, hop: int, step: int, frame_len: int, first: int, row_len: int) -> np.ndarray:
    """The greedy pass over one row's candidates, on the host."""
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
    packed = _candidates(power, floor, index, hop, N, osr, k, sw0, sw1, thresh_db)
    packed = packed.cpu().numpy()  # the one synchronisation
    return _greedy(packed, hop, step, frame_len, first, row_len)


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
        return starts_t, _no_frames(frame_symbols, dev)
    # (the finder only accepts frames that fit the stream, so the gather needs no second check)
    return starts_t, plan.run(_gather(iq, starts_t, frame_len))


def _no_frames(frame_symbols: int, dev: torch.device) -> DemodResult:
    return DemodResult(symbols=torch.empty((0, int(frame_symbols)), dtype=torch.uint16, device=dev),
                       sync=torch.empty(0, dtype=torch.uint8, device=dev),
                       cfo=torch.empty(0, dtype=torch.float32, device=dev),
                       time_offset=torch.empty(0, dtype=torch.float32, device=dev),
                       max_amp=torch.empty(0, dtype=torch.float32, device=dev))


def lowpass_taps(ntaps: int, cutoff: float, gain: float = 1.0) -> np.ndarray:
    """A Hamming-windowed sinc low-pass for ``Channelizer``: float32 [ntaps],
    ``2*cutoff*sinc(2*cutoff*(j - (ntaps-1)/2)) * hamming(ntaps)`` computed in double, divided by
    its sum (unit gain at the channel centre) and multiplied by ``gain``, still in double, then
    rounded to fp32.  ``cutoff`` is in cycles per sample of the rate the taps run at, ``0 < cutoff
    <= 0.5``: the input rate, or for a rational bank ``interp`` times it - there ``gain=interp``
    makes up for the zero-stuffing and ``cutoff`` is usually ``0.5 / decim``."""
    ntaps, cutoff, gain = int(ntaps), float(cutoff), float(gain)
    if ntaps < 1:
        raise ValueError("ntaps must be >= 1")
    if not 0.0 < cutoff <= 0.5:
        raise ValueError("cutoff must be in (0, 0.5] cycles per sample")
    j = np.arange(ntaps, dtype=np.float64)
    h = 2.0 * cutoff * np.sinc(2.0 * cutoff * (j - (ntaps - 1) / 2.0)) * np.hamming(ntaps)
    h = h / h.sum()
    return (h if gain == 1.0 else h * gain).astype(np.float32)


def nco_table(period: int) -> np.ndarray:
    """The oscillator table ``Channelizer`` uses: ``exp(-2 pi i m / period)``, m = 0 .. period-1,
    cosine and sine computed in double and rounded to fp32 (complex64 [period])."""
    ang = -2.0 * np.pi * np.arange(int(period), dtype=np.float64) / int(period)
    w = np.empty(int(period), np.complex64)
    w.real = np.cos(ang).astype(np.float32)
    w.imag = np.sin(ang).astype(np.float32)
    return w


# raw sample dtypes: (LORA_IQ_* format, default scale before its rounding to fp32, bias)
_RAW = {torch.int16: (_capi.LORA_IQ_CS16, 1.0 / 32768.0, 0.0),
        torch.int8: (_capi.LORA_IQ_CS8, 1.0 / 128.0, 0.0),
        torch.uint8: (_capi.LORA_IQ_CU8, 1.0 / 127.5, 127.5)}


def _is_raw(iq) -> bool:
    """An integer tensor: to be taken as raw samples (and refused if it is not a valid one)."""
    return isinstance(iq, torch.Tensor) and not (iq.dtype.is_complex or iq.dtype.is_floating_point)


def _raw_format(dtype):
    if dtype not in _RAW:
        raise TypeError(f"raw samples are int16 (cs16), int8 (cs8) or uint8 (cu8) tensors, not {dtype}")
    return _RAW[dtype]


def raw_scale(dtype) -> float:
    """The default ``scale`` of a raw sample dtype, rounded to fp32: 1/32768 for ``torch.int16``,
    1/128 for ``torch.int8``, 1/127.5 for ``torch.uint8``."""
    return float(np.float32(_raw_format(dtype)[1]))


def _scale_of(dtype, scale) -> float:
    return raw_scale(dtype) if scale is None else float(np.float32(scale))


def raw_to_complex(raw: torch.Tensor, scale: Optional[float] = None) -> torch.Tensor:
    """Raw samples ``[.., 2]`` (``int16``, ``int8`` or ``uint8``; I, Q) as complex64 ``[..]`` on the
    tensor's device, by this module's definition in torch operations: ``(float(v) - bias) *
    scale``, each operation rounded once to fp32, ``bias`` 127.5 for ``uint8`` and none otherwise;
    ``scale`` (default ``raw_scale(raw.dtype)``) is rounded to fp32 and not checked.  Bit for bit
    what the banks' kernels make of the same tensor."""
    if not isinstance(raw, torch.Tensor) or raw.dim() < 1 or raw.shape[-1] != 2:
        raise ValueError("raw samples are a [.., 2] integer tensor (I, Q)")
    _, _, bias = _raw_format(raw.dtype)
    x = raw.to(torch.float32)
    if bias:
        x = x - bias
    x = x * _scale_of(raw.dtype, scale)
    return torch.view_as_complex(x.contiguous())


def _check_raw(raw: torch.Tensor, device: torch.device):
    """``(rows, row_len, row_stride in samples, format)`` of a raw [L, 2] or [R, L, 2] tensor after
    everything the C library cannot check about a pointer."""
    _require_cuda(raw, "iq")
    if raw.device != device:
        raise ValueError(f"iq is on {raw.device}, the channelizer is on {device}")
    fmt = _raw_format(raw.dtype)[0]
    if raw.dim() not in (2, 3) or raw.shape[-1] != 2:
        raise ValueError("raw samples are a [L, 2] or [R, L, 2] integer tensor (I, Q)")
    if raw.dim() == 2:
        raw = raw.unsqueeze(0)
    R, L, _ = raw.shape
    if raw.stride(2) != 1 or (L > 1 and raw.stride(1) != 2):
        raise ValueError("raw samples must have unit stride over (I, Q) and stride 2 over the samples")
    if R > 1 and (raw.stride(0) % 2 or raw.stride(0) < 2 * L):
        raise ValueError("raw rows must be an even number of elements apart and must not overlap")
    return R, L, (raw.stride(0) // 2 if R > 1 else L), fmt


class Channelizer:
    """A digital down-converter bank on the GPU: one wideband stream in, ``C = len(steps)``
    channel streams out, each mixed down from ``steps[c] / period`` cycles per input sample above
    the tuner, low-pass filtered with the real ``taps`` and resampled by ``interp / decim``.  One
    kernel reads the wideband data once.  With ``interp == 1`` it is lora_channelize_batch: the
    taps run at the input rate and every ``decim``-th filter output is kept.  With ``interp > 1``
    it is lora_resample_channelize_batch, the polyphase interpolate-by-``interp``,
    decimate-by-``decim`` bank: the taps are a prototype filter at ``interp`` times the input rate
    (``lowpass_taps(ntaps, 0.5 / decim, gain=interp)``).  The arithmetic of both is defined
    exactly in include/lora_mi355x.h (the definitions are this library's own: the reference has
    no channelizer), so a host restatement reproduces every bit.

    Limits: channel centres are multiples of ``fs / period``; the input rate must be ``bw * osr
    * decim / interp`` of the demodulator that follows; ``period`` 1..4096, 1..32 channels; with
    ``interp == 1`` ``decim`` 1..64 and 1..512 taps; with ``interp`` 2..16 ``decim`` ``interp``..256
    (a rate-reducing bank only) and 1..4096 taps with ``ceil(ntaps / interp) <= 512``.  Ratios
    beyond those (2.048 MS/s to 125 kS/s is 125/2048) are not covered.

    The taps and the oscillator table (``nco_table(period)``) are kept on the device.
    ``delay`` is the filter's group delay, ``(ntaps - 1) / (2 * interp)`` input samples.

    ``run`` also takes raw integer samples (this module's docstring): the same kernel converts
    them as it loads them, by ``raw_to_complex``'s arithmetic, and everything else is unchanged."""

    def __init__(self, decim: int, taps, period: int, steps, device=None, interp: int = 1):
        self.decim, self.period, self.interp = int(decim), int(period), int(interp)
        h = np.ascontiguousarray(taps, np.float32)
        self.steps = [int(k) for k in steps]
        if not 1 <= self.interp <= 16:
            raise ValueError("interp must be in 1..16")
        if self.interp == 1:
            if not 1 <= self.decim <= 64:
                raise ValueError("decim must be in 1..64")
            if h.ndim != 1 or not 1 <= h.shape[0] <= 512:
                raise ValueError("taps must be 1..512 real values")
        else:
            if not self.interp <= self.decim <= 256:
                raise ValueError("with interp > 1, decim must be in interp..256 (a rate-reducing bank only)")
            if h.ndim != 1 or not 1 <= h.shape[0] <= 4096 or -(-h.shape[0] // self.interp) > 512:
                raise ValueError("taps must be 1..4096 real values, at most 512 per interpolation phase")
        if not 1 <= self.period <= 4096:
            raise ValueError("period must be in 1..4096")
        if not 1 <= len(self.steps) <= 32 or any(abs(k) >= 1 << 31 for k in self.steps):
            raise ValueError("steps must be 1..32 ints")
        self.ntaps, self.channels = int(h.shape[0]), len(self.steps)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise TypeError("Channelizer runs on a CUDA (HIP) device; there is no CPU fallback")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._lib = _capi.lib()
        self._steps = (_capi.C.c_int32 * self.channels)(*self.steps)
        self.taps = torch.from_numpy(h.copy()).to(self.device)
        self.nco = torch.from_numpy(nco_table(self.period)).to(self.device)

    @property
    def delay(self) -> float:
        return (self.ntaps - 1) / (2 * self.interp)

    def _outputs(self, L: int) -> int:
        if self.interp == 1:
            return 0 if L < self.ntaps else (L - self.ntaps) // self.decim + 1
        span = (L - 1) * self.interp + 1
        return 0 if L < 1 or span < self.ntaps else (span - self.ntaps) // self.decim + 1

    def outputs(self, L: int) -> int:
        """Outputs per channel for a row of ``L`` samples.  ``interp == 1``: ``0 if L < ntaps else
        (L - ntaps) // decim + 1`` (lora_channelize_outputs).  Otherwise, with ``span = (L - 1) *
        interp + 1``: ``0 if L < 1 or span < ntaps else (span - ntaps) // decim + 1``
        (lora_resample_outputs)."""
        if self.interp == 1:
            return _capi.check(self._lib.lora_channelize_outputs(int(L), self.ntaps, self.decim))
        return _capi.check(self._lib.lora_resample_outputs(int(L), self.ntaps, self.interp, self.decim))

    def run(self, iq: torch.Tensor, first_sample: int = 0, out: Optional[torch.Tensor] = None,
            scale: Optional[float] = None) -> torch.Tensor:
        """Channelize a [L] complex64 CUDA stream into [C, W], or [R, L] rows (a strided view with
        non-overlapping rows is accepted, as for ``DemodPlan.scan``) into [R, C, W]; ``W =
        outputs(L)``.  Or raw samples: an ``int16``, ``int8`` or ``uint8`` CUDA tensor [L, 2], or
        [R, L, 2] rows (unit stride over I, Q, stride 2 over the samples, rows any even number of
        elements apart that does not make them overlap; any slice ``raw[k:]`` will do, the kernel
        needs no alignment beyond one sample), converted in the kernel with ``scale`` (default
        ``raw_scale(iq.dtype)``; ``scale`` with a complex64 input is a ``ValueError``).  ``first_sample`` (>= 0) is the index of ``iq[.., 0]`` in the recording, which
        keeps the oscillators' phase continuous across chunks: a chunk that starts at a multiple of
        ``decim`` and overlaps its predecessor by ``ntaps - decim`` samples continues its outputs
        (with ``interp > 1``: a chunk that starts at a sample ``n0`` with ``n0 * interp`` a multiple
        of ``decim``, after a predecessor long enough to hold the ``n0 * interp / decim`` outputs
        before it).
        ``out``: a contiguous complex64 [C, >= W] (or [R, C, >= W]) tensor to write into; its
        columns from W on are left alone and the [.., :W] view is returned.  One kernel on the
        current stream, nothing allocated besides the output, so the call can be captured in a
        HIP graph."""
        raw = _is_raw(iq)
        if raw:
            one = iq.dim() == 2
            R, L, row_stride, fmt = _check_raw(iq, self.device)
            scale = _scale_of(iq.dtype, scale)
        else:
            if scale is not None:
                raise ValueError("scale belongs to raw integer samples; a complex64 input has none")
            one = isinstance(iq, torch.Tensor) and iq.dim() == 1
            iq = _check_iq(iq, self.device)
            R, L = iq.shape
            row_stride = iq.stride(0) if R > 1 else L
        first_sample = int(first_sample)
        if first_sample < 0:
            raise ValueError("first_sample must be >= 0")
        W = self._outputs(L)
        C = self.channels
        if out is None:
            out = torch.empty((C, W) if one else (R, C, W), dtype=torch.complex64, device=self.device)
        else:
            _require_cuda(out, "out")
            want = (C,) if one else (R, C)
            if out.dtype != torch.complex64:
                raise TypeError("out must be complex64")
            if (out.device != self.device or out.dim() != len(want) + 1 or tuple(out.shape[:-1]) != want
                    or out.shape[-1] < W or not out.is_contiguous()):
                raise ValueError(f"out must be a contiguous complex64 {list(want) + ['>=%d' % W]} tensor on "
                                 f"{self.device}")
        if R == 0 or W == 0:
            return out[..., :W]  # nothing to launch (and an empty tensor has no address to pass)
        # the rational entry is the integer one with interp in front of decim; a raw entry is its
        # float counterpart with the format and the scale behind iq
        lib = self._lib
        if self.interp == 1:
            entry, rates = (lib.lora_channelize_raw_batch if raw else lib.lora_channelize_batch), (self.decim,)
        else:
            entry = lib.lora_resample_channelize_raw_batch if raw else lib.lora_resample_channelize_batch
            rates = (self.interp, self.decim)
        src = (iq.data_ptr(), fmt, scale) if raw else (iq.data_ptr(),)
        got = _capi.check(entry(
            *src, R, L, row_stride, first_sample, self.taps.data_ptr(), self.ntaps,
            *rates, self.nco.data_ptr(), self.period, self._steps, C, out.data_ptr(), out.shape[-1],
            self.device.index, _stream_handle(self.device)))
        assert got == W, (got, W)
        return out[..., :W]


def receive_wideband(plan: DemodPlan, chan: Channelizer, iq: torch.Tensor, frame_symbols: int,
                     hop: Optional[int] = None, sync: int = 0x12, thresh_db: float = 0.0,
                     scale: Optional[float] = None) -> Tuple[torch.Tensor, torch.Tensor, DemodResult]:
    """``receive`` for a wideband capture: channelize the [L] complex64 CUDA stream ``iq`` (or the
    raw [L, 2] integer stream, converted with ``scale`` as ``Channelizer.run`` does) with
    ``chan``, scan all channel rows at once, find the frames of ``frame_symbols`` data symbols in
    each row by the finder's rule, gather them and demodulate them.

    Returns ``(channel, starts, result)``: int64 [K] tensors on the plan's device, ordered by
    channel and then by start, and ``plan.run``'s DemodResult for the K frames.  Starts are in
    CHANNEL samples: frame i began near wideband sample ``starts[i] * chan.decim / chan.interp +
    chan.delay``.

    The plan's constraints are ``receive``'s (``dechirp=True``, bw 125 kHz).  Its ``step`` must
    match the channel rate - the wideband rate must be ``bw * osr * chan.decim / chan.interp`` -
    which is the caller's responsibility: nothing here can check it.  The work is one
    ``Channelizer.run``, one ``plan.scan`` over the [C, W] rows, one gather and one ``plan.run``; the candidates of all
    rows come to the host in one copy, so there is one synchronisation, as in ``receive``.  With
    no frame found the tensors are empty and no demod call is made."""
    if not plan.dechirp:
        raise ValueError("receive_wideband needs a plan with dechirp=True: the finder reads dechirped peaks")
    if not isinstance(iq, torch.Tensor) or iq.dim() != (2 if _is_raw(iq) else 1):
        raise ValueError("receive_wideband takes one [L] stream (raw samples: [L, 2])")
    if chan.device != plan.device:
        raise ValueError(f"the channelizer is on {chan.device}, the plan is on {plan.device}")
    hop = plan.step // 4 if hop is None else int(hop)
    N, step, k, sw0, sw1, frame_len = _geometry(hop, plan.sf, plan.osr, frame_symbols, sync, plan.bw)
    rows = chan.run(iq, scale=scale)  # [C, Wc]
    C, Wc = rows.shape
    dev = plan.device
    found = []
    if Wc >= step:  # (scan of shorter rows has no window)
        met = plan.scan(rows, hop)
        if met.power.shape[1] > k:
            packed = _candidates(met.power, met.power_avg, met.index, hop, N, step // N, k, sw0, sw1, thresh_db)
            packed = packed.cpu().numpy()  # the one synchronisation
            found = [_greedy(packed[c], hop, step, frame_len, 0, Wc) for c in range(C)]
    K = sum(len(s) for s in found)
    if K == 0:
        empty = torch.empty(0, dtype=torch.int64, device=dev)
        return empty, empty.clone(), _no_frames(frame_symbols, dev)
    channel = np.repeat(np.arange(C, dtype=np.int64), [len(s) for s in found])
    starts = np.concatenate(found)
    channel_t, starts_t = torch.from_numpy(channel).to(dev), torch.from_numpy(starts).to(dev)
    # the rows are one contiguous [C * Wc] stream; the finder only accepts frames inside their row
    frames = _gather(rows.reshape(-1), channel_t * Wc + starts_t, frame_len)
    return channel_t, starts_t, plan.run(frames)



@dataclass
class FoundFrames:
    """What ``find_frames_device`` leaves on the device for R rows with ``capacity`` slots each."""

    count: torch.Tensor   # [R] int32            frames the pass accepted (may exceed capacity)
    starts: torch.Tensor  # [R, capacity] int64  the first min(count, capacity) starts, then -1
    end: torch.Tensor     # [R] int64            ``first`` as the pass left it: the next chunk's, once shifted

    @property
    def valid(self) -> torch.Tensor:
        """bool [R, capacity]: ``arange(capacity) < count[:, None]`` - the slots that hold a frame."""
        return torch.arange(self.starts.shape[1], device=self.count.device) < self.count[:, None]


@dataclass
class StreamFrames:
    """``receive_device``'s result: the found frames and the demodulation of every slot,
    ``result`` having ``F = R * capacity`` frames in row-major order (slot j of row r is frame
    ``r * capacity + j``).  Only the slots of ``found.valid`` mean anything."""

    found: FoundFrames
    result: DemodResult


def _find_first(first, R: int, dev: torch.device) -> Optional[torch.Tensor]:
    """``first`` as the entry takes it: None (0 in every row) or an int64 [R] tensor."""
    if first is None:
        return None
    if isinstance(first, torch.Tensor):
        if first.dtype != torch.int64:
            raise TypeError(f"first must be an int64 tensor, got {first.dtype}")
        if first.dim() != 1 or first.shape[0] != R:
            raise ValueError(f"first must be one int per row: an int64 [{R}] tensor")
        return first
    first = int(first)
    if first < 0:
        raise ValueError("first must be >= 0")
    return torch.full((R,), first, dtype=torch.int64, device=dev) if first and R else None


def find_frames_device(metrics: DetectMetrics, hop: int, sf: int, osr: int, frame_symbols: int, sync: int = 0x12,
                       thresh_db: float = 0.0, first: Union[None, int, torch.Tensor] = None,
                       row_len: Optional[int] = None, capacity: Optional[int] = None,
                       out: Optional[FoundFrames] = None, bw: int = 125000) -> FoundFrames:
    """``find_frames`` as one kernel (lora_find_frames_batch): the frame starts of every scanned row
    by the rule in this module's docstring, left on the device.  Nothing is copied to the host
    and nothing synchronises.

    ``metrics``: ``DemodPlan.scan``'s CUDA result for one row ([W]) or R rows ([R, W]; rows may be
    strided as ``scan``'s ``out=`` allows, power, power_avg and index sharing one row stride).
    ``first``: no frame starts before this sample - None (0), an int for every row, or an int64
    [R] tensor on the metrics' device, which is how a chunked caller carries the previous chunk's
    ``end`` without reading it.  ``row_len`` as for ``find_frames``.  ``capacity``: slots per row
    (default ``row_len // frame_len``, which bounds what a row can hold, so nothing is dropped);
    with a smaller one ``count`` still counts every accepted frame and ``count > capacity`` tells
    that some were not stored.  ``out``: a FoundFrames of contiguous tensors to write into (count
    int32 [R], starts int64 [R, capacity], end int64 [R]).

    Returns FoundFrames (R = 1 for a [W] input).  All of it is fully written, also for rows with
    no window to test (count 0, ``end = first``).  One kernel on the current stream; nothing is
    allocated besides the outputs and, for an int ``first`` other than 0, its [R] tensor.
    ``ValueError``: as ``find_frames``, and a ``first`` tensor that is not [R]; ``TypeError``: a
    ``first`` tensor that is not int64, metrics of the wrong dtype or not on a CUDA device."""
    N, step, k, sw0, sw1, frame_len = _geometry(hop, sf, osr, frame_symbols, sync, bw)
    hop, osr = int(hop), step // N
    power, floor, index = metrics.power, metrics.power_avg, metrics.index
    if not all(isinstance(t, torch.Tensor) for t in (power, floor, index)):
        raise TypeError("find_frames_device needs metrics with power, power_avg and index")
    if power.dim() == 1:
        power, floor, index = power.unsqueeze(0), floor.unsqueeze(0), index.unsqueeze(0)
    if power.dim() != 2 or floor.shape != power.shape or index.shape != power.shape:
        raise ValueError("find_frames_device takes power, power_avg and index of one [W] or [R, W] shape")
    if power.dtype != torch.float32 or floor.dtype != torch.float32 or index.dtype != torch.uint16:
        raise TypeError("power and power_avg must be float32 and index uint16")
    R, W = power.shape
    first_t = _find_first(first, R, power.device)
    if row_len is None:
        row_len = (W - 1) * hop + step if W else 0
    row_len = int(row_len)
    capacity = row_len // frame_len if capacity is None else int(capacity)
    if row_len < 0 or capacity < 0:
        raise ValueError("row_len and capacity must be >= 0")
    for t, name in ((power, "power"), (floor, "power_avg"), (index, "index")):
        _require_cuda(t, "metrics." + name)
    dev = power.device
    if floor.device != dev or index.device != dev or (first_t is not None and first_t.device != dev):
        raise ValueError(f"power_avg, index and first must be on {dev}, where power is")
    if W > 1 and any(t.stride(1) != 1 for t in (power, floor, index)):
        raise ValueError("the metrics must have unit column stride")
    strides = {t.stride(0) for t in (power, floor, index)} if R > 1 else {W}
    if len(strides) != 1 or min(strides) < W:
        raise ValueError("power, power_avg and index must share one row stride >= W")
    if out is None:
        out = FoundFrames(count=torch.empty(R, dtype=torch.int32, device=dev),
                          starts=torch.empty((R, capacity), dtype=torch.int64, device=dev),
                          end=torch.empty(R, dtype=torch.int64, device=dev))
    else:
        for name, dt, shape in (("count", torch.int32, (R,)), ("starts", torch.int64, (R, capacity)),
                                ("end", torch.int64, (R,))):
            t = getattr(out, name)
            _require_cuda(t, "out." + name)
            if t.dtype != dt:
                raise TypeError(f"out.{name} must be {dt}, got {t.dtype}")
            if t.device != dev or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"out.{name} must be a contiguous {dt} {list(shape)} tensor on {dev}")
    if R == 0:
        return out
    if first_t is not None and not first_t.is_contiguous():
        first_t = first_t.contiguous()
    prm = _capi.FindParams(int(sf), osr, int(sync) & 0xFF, float(thresh_db), hop, int(frame_symbols), dev.index)
    got = _capi.check(_capi.lib().lora_find_frames_batch(
        _capi.C.byref(prm), power.data_ptr(), floor.data_ptr(), index.data_ptr(), R, W, strides.pop(),
        first_t.data_ptr() if first_t is not None else None, row_len, capacity,
        out.starts.data_ptr() if capacity else None, out.count.data_ptr(), out.end.data_ptr(), _stream_handle(dev)))
    assert got == R, (got, R)
    return out


def _receive_rows(plan: DemodPlan, rows: torch.Tensor, frame_symbols, hop, sync, thresh_db, first,
                  capacity) -> StreamFrames:
    """Scan, find, gather and demodulate the [R, L] rows (checked by the caller) on the device."""
    hop = plan.step // 4 if hop is None else int(hop)
    frame_len = _geometry(hop, plan.sf, plan.osr, frame_symbols, sync, plan.bw)[-1]
    R, L = rows.shape
    dev = plan.device
    if L >= plan.step:
        met = plan.scan(rows, hop)
    else:  # (no window: nothing to scan, and the finder only has its outputs to fill)
        met = DetectMetrics(*(torch.empty((R, 0), dtype=dt, device=dev)
                              for dt in (torch.float32, torch.float32, torch.float32, torch.uint16)))
    found = find_frames_device(met, hop, plan.sf, plan.osr, frame_symbols, sync, thresh_db, first, L, capacity,
                               None, plan.bw)
    cap = found.starts.shape[1]
    if R * cap == 0:
        return StreamFrames(found, _no_frames(frame_symbols, dev))
    if L < frame_len:
        raise ValueError(f"rows of {L} samples hold no frame of {frame_len}: capacity must be 0")
    # the rows as one stream (row r begins at r * row stride); an empty slot (-1) reads its row's
    # first frame_len samples
    rs = rows.stride(0) if R > 1 else L
    flat = rows.as_strided(((R - 1) * rs + L,), (1,))
    at = found.starts.clamp_min(0) + (torch.arange(R, device=dev) * rs)[:, None]
    return StreamFrames(found, plan.run(_gather(flat, at.reshape(-1), frame_len)))


def receive_device(plan: DemodPlan, iq: torch.Tensor, frame_symbols: int, hop: Optional[int] = None,
                   sync: int = 0x12, thresh_db: float = 0.0, first: Union[None, int, torch.Tensor] = None,
                   capacity: Optional[int] = None) -> StreamFrames:
    """``receive`` without the host: ``plan.scan``, ``find_frames_device``, one gather and one
    ``plan.run``, with nothing read back in between - no synchronisation, every shape computed
    from host integers.  ``iq`` is a [L] stream or [R, L] rows (complex64 CUDA, rows laid out as
    ``scan`` takes them); ``first`` and ``capacity`` are ``find_frames_device``'s, ``row_len`` is L.

    Returns StreamFrames: ``found`` (count [R], starts [R, capacity], end [R]) and ``result``, the
    DemodResult of ALL ``R * capacity`` slots, row-major.  The slots of ``found.valid`` hold what
    ``receive`` returns for the same stream, bit for bit.  A slot beyond its row's count holds
    the demodulation of the row's first ``frame_len`` samples: defined input, nothing
    uninitialised is read, and the result means nothing - select with ``found.valid``.
    (``symbols`` is uint16, which torch does not index on the device: select from
    ``symbols.to(torch.int32)``, or after the copy to the host.)

    ``capacity`` defaults to ``L // frame_len``, so the gathered frames are as large as the
    stream itself and every slot is demodulated; a caller who knows their traffic passes a
    smaller one and watches ``found.count > capacity`` for frames that were found but not kept.
    A row shorter than ``frame_len`` gives capacity 0 and no demod call.  Chunked: the next
    chunk's ``first`` is ``(found.end - advance).clamp_min(0)``, a tensor operation, so chunk b + 1
    can be enqueued before anyone reads chunk b's count."""
    if not plan.dechirp:
        raise ValueError("receive_device needs a plan with dechirp=True: the finder reads dechirped peaks")
    if not isinstance(iq, torch.Tensor) or iq.dim() not in (1, 2):
        raise ValueError("receive_device takes one [L] stream or [R, L] rows")
    hop = plan.step // 4 if hop is None else int(hop)
    _geometry(hop, plan.sf, plan.osr, frame_symbols, sync, plan.bw)
    return _receive_rows(plan, _check_iq(iq, plan.device), frame_symbols, hop, sync, thresh_db, first, capacity)


def receive_wideband_device(plan: DemodPlan, chan: "Channelizer", iq: torch.Tensor, frame_symbols: int,
                            hop: Optional[int] = None, sync: int = 0x12, thresh_db: float = 0.0,
                            scale: Optional[float] = None, first: Union[None, int, torch.Tensor] = None,
                            capacity: Optional[int] = None) -> StreamFrames:
    """``receive_wideband`` without the host: ``chan.run`` on the [L] complex64 stream (or the raw
    [L, 2] integer stream, converted with ``scale``), then ``receive_device`` over the [C, Wc]
    channel rows - row r of the result is channel r, slot j of channel r is frame ``r * capacity +
    j`` of ``result``.  Starts are in CHANNEL samples, as ``receive_wideband``'s; ``first`` ([C], in
    channel samples) and ``capacity`` are ``find_frames_device``'s with ``row_len = Wc``.  The valid
    slots, taken channel by channel, are ``receive_wideband``'s frames in its order.  No
    synchronisation; everything said of ``receive_device``'s slots and capacity holds here."""
    if not plan.dechirp:
        raise ValueError("receive_wideband_device needs a plan with dechirp=True: the finder reads dechirped peaks")
    if not isinstance(iq, torch.Tensor) or iq.dim() != (2 if _is_raw(iq) else 1):
        raise ValueError("receive_wideband_device takes one [L] stream (raw samples: [L, 2])")
    if chan.device != plan.device:
        raise ValueError(f"the channelizer is on {chan.device}, the plan is on {plan.device}")
    hop = plan.step // 4 if hop is None else int(hop)
    _geometry(hop, plan.sf, plan.osr, frame_symbols, sync, plan.bw)
    rows = chan.run(iq, scale=scale)  # [C, Wc]
    return _receive_rows(plan, rows, frame_symbols, hop, sync, thresh_db, first, capacity)


@dataclass
class StreamPackets:
    """``receive_frames_device``'s result for R rows with ``capacity`` slots each; ``result`` and
    ``frames`` hold all ``R * capacity`` slots in row-major order (slot j of row r is frame
    ``r * capacity + j``).  Only the slots of ``found.valid`` mean anything."""

    found: FoundFrames        # count [R], starts [R, capacity], end [R]: as find_frames_device's
    nsym: torch.Tensor        # [R, capacity] int32: each frame's data symbols by its header, 0 in empty slots
    result: DemodResult       # of every slot cut to (2 + max_symbols) * step, zeros after its frame
    frames: "object"          # codec.FrameResult of every slot: status, nbytes, rdd, has_crc, errors, payload
    candidates: torch.Tensor  # [R] int32: candidates listed per row (above cand_capacity: some were dropped)
    llr: Optional[torch.Tensor] = None  # soft=True: [R * capacity, 2 + max_symbols, sf] soft bits of the slots
    cfo_bins: Optional[torch.Tensor] = None  # receive_preamble_frames_device: [R, capacity] int32 offsets in bins


def _scan_rows(metrics: DetectMetrics, what: str):
    """power, power_avg, index as [R, W] and their shared row stride, checked as the finder needs."""
    power, floor, index = metrics.power, metrics.power_avg, metrics.index
    if not all(isinstance(t, torch.Tensor) for t in (power, floor, index)):
        raise TypeError(f"{what} needs metrics with power, power_avg and index")
    if power.dim() == 1:
        power, floor, index = power.unsqueeze(0), floor.unsqueeze(0), index.unsqueeze(0)
    if power.dim() != 2 or floor.shape != power.shape or index.shape != power.shape:
        raise ValueError(f"{what} takes power, power_avg and index of one [W] or [R, W] shape")
    if power.dtype != torch.float32 or floor.dtype != torch.float32 or index.dtype != torch.uint16:
        raise TypeError("power and power_avg must be float32 and index uint16")
    for t, name in ((power, "power"), (floor, "power_avg"), (index, "index")):
        _require_cuda(t, "metrics." + name)
    R, W = power.shape
    if floor.device != power.device or index.device != power.device:
        raise ValueError(f"power_avg and index must be on {power.device}, where power is")
    if W > 1 and any(t.stride(1) != 1 for t in (power, floor, index)):
        raise ValueError("the metrics must have unit column stride")
    strides = {t.stride(0) for t in (power, floor, index)} if R > 1 else {W}
    if len(strides) != 1 or min(strides) < W:
        raise ValueError("power, power_avg and index must share one row stride >= W")
    return power, floor, index, strides.pop()


def find_candidates_device(metrics: DetectMetrics, hop: int, sf: int, osr: int, sync: int = 0x12,
                           thresh_db: float = 0.0, row_len: Optional[int] = None,
                           cand_capacity: Optional[int] = None, bw: int = 125000):
    """The finder's candidates, listed on the device (lora_find_candidates_batch, one kernel): the
    candidate rule and refinement of this module's docstring, unchanged, and per row, in
    increasing w, every refined start with ``start >= 0`` and ``start + 10 * step <= row_len``
    (two sync symbols and a header fit) that differs from the row's last listed one.

    Returns ``(count, starts)``: int32 [R] - the starts listed, which may exceed the capacity -
    and int64 [R, cand_capacity], -1 beyond the count.  ``cand_capacity`` defaults to
    ``ceil(row_len / (4 * step))``.  Nothing synchronises."""
    N, step, k, sw0, sw1, head_len = _geometry(hop, sf, osr, 8, sync, bw)
    hop, osr = int(hop), step // N
    power, floor, index, stride = _scan_rows(metrics, "find_candidates_device")
    R, W = power.shape
    if row_len is None:
        row_len = (W - 1) * hop + step if W else 0
    row_len = int(row_len)
    cap = _ceil_div(row_len, 4 * step) if cand_capacity is None else int(cand_capacity)
    if row_len < 0 or cap < 0:
        raise ValueError("row_len and cand_capacity must be >= 0")
    dev = power.device
    count = torch.empty(R, dtype=torch.int32, device=dev)
    starts = torch.empty((R, cap), dtype=torch.int64, device=dev)
    if R:
        prm = _capi.FindParams(int(sf), osr, int(sync) & 0xFF, float(thresh_db), hop, 8, dev.index)
        _capi.check(_capi.lib().lora_find_candidates_batch(
            _capi.C.byref(prm), power.data_ptr(), floor.data_ptr(), index.data_ptr(), R, W, stride, row_len, cap,
            starts.data_ptr() if cap else None, count.data_ptr(), _stream_handle(dev)))
    return count, starts


def select_frames_device(cand_starts: torch.Tensor, status: torch.Tensor, nsym: torch.Tensor, step: int,
                         row_len: int, max_symbols: int, first: Union[None, int, torch.Tensor] = None,
                         capacity: Optional[int] = None) -> Tuple[FoundFrames, torch.Tensor]:
    """The greedy pass over candidates whose headers were decoded (lora_select_frames_batch, one
    kernel).  ``cand_starts`` int64, ``status`` and ``nsym`` int32, all [R, C] and contiguous on
    one device: ``find_candidates_device``'s starts and ``codec.decode_header``'s results for the
    frame cut at each.  In slot order, slot j is accepted when its status is FRAME_OK, ``nsym <=
    max_symbols``, ``start >= first`` (an empty slot, -1, never is) and ``start + (2 + nsym) *
    step <= row_len``; ``first`` then becomes that end.  ``first`` and ``capacity`` as
    ``find_frames_device``'s (capacity defaults to ``row_len // (10 * step)``).

    Returns ``(found, nsym)``: a FoundFrames of the same meaning, and int32 [R, capacity], each
    accepted frame's data symbols, 0 in empty slots.  Nothing synchronises."""
    for t, name, dt in ((cand_starts, "cand_starts", torch.int64), (status, "status", torch.int32),
                        (nsym, "nsym", torch.int32)):
        _require_cuda(t, name)
        if t.dtype != dt:
            raise TypeError(f"{name} must be {dt}, got {t.dtype}")
        if t.dim() != 2 or t.shape != cand_starts.shape or t.device != cand_starts.device or not t.is_contiguous():
            raise ValueError("cand_starts, status and nsym must be contiguous [R, C] tensors on one device")
    R, C = cand_starts.shape
    dev = cand_starts.device
    step, row_len, max_symbols = int(step), int(row_len), int(max_symbols)
    first_t = _find_first(first, R, dev)
    if first_t is not None and first_t.device != dev:
        raise ValueError(f"first must be on {dev}")
    capacity = row_len // (10 * step) if capacity is None else int(capacity)
    if capacity < 0:
        raise ValueError("capacity must be >= 0")
    found = FoundFrames(count=torch.empty(R, dtype=torch.int32, device=dev),
                        starts=torch.empty((R, capacity), dtype=torch.int64, device=dev),
                        end=torch.empty(R, dtype=torch.int64, device=dev))
    out_nsym = torch.empty((R, capacity), dtype=torch.int32, device=dev)
    if R:
        if first_t is not None and not first_t.is_contiguous():
            first_t = first_t.contiguous()
        _capi.check(_capi.lib().lora_select_frames_batch(
            cand_starts.data_ptr() if C else None, status.data_ptr() if C else None, nsym.data_ptr() if C else None,
            R, C, first_t.data_ptr() if first_t is not None else None, row_len, step, max_symbols, capacity,
            found.starts.data_ptr() if capacity else None, out_nsym.data_ptr() if capacity else None,
            found.count.data_ptr(), found.end.data_ptr(), dev.index, _stream_handle(dev)))
    return found, out_nsym


def _receive_frame_rows(plan: DemodPlan, rows: torch.Tensor, max_symbols, hop, sync, thresh_db, first, capacity,
                        cand_capacity, soft: bool = False, max_flips: int = 5) -> StreamPackets:
    """The nine steps of ``receive_frames_device`` on [R, L] rows (checked by the caller); with
    ``soft`` the two decodes run on soft bits, columns 2 - 9 (the header's) reduced."""
    from . import codec

    sf, step, dev = plan.sf, plan.step, plan.device
    max_symbols = int(max_symbols)
    if sf < codec.FRAME_MIN_SF:
        raise ValueError("self-describing frames need SF 7-12")
    if max_symbols < 8:
        raise ValueError("max_symbols must be >= 8: a frame has at least its header's eight symbols")
    R, L = rows.shape
    head_len, cut = 10 * step, (2 + max_symbols) * step
    if L >= step:
        met = plan.scan(rows, hop)
    else:  # (no window: nothing to scan, and the kernels only have their outputs to fill)
        met = DetectMetrics(*(torch.empty((R, 0), dtype=dt, device=dev)
                              for dt in (torch.float32, torch.float32, torch.float32, torch.uint16)))
    ccount, cstarts = find_candidates_device(met, hop, sf, plan.osr, sync, thresh_db, L, cand_capacity, plan.bw)
    C = cstarts.shape[1]
    # the rows as one stream (row r begins at r * row stride); an empty slot stays negative
    rs = rows.stride(0) if R > 1 else L
    flat = rows.as_strided(((R - 1) * rs + L,), (1,)) if R else rows.reshape(-1)
    row0 = (torch.arange(R, device=dev) * rs)[:, None]
    if R * C:
        at = torch.where(cstarts >= 0, cstarts + row0, cstarts).reshape(-1)
        heads = gather_frames_device(flat, at, torch.full_like(at, head_len), head_len)
        if soft:
            hdr = codec.decode_header_soft(plan.soft_bits(heads, plan.run(heads), reduced=(2, 8))[:, 2:], sf,
                                           max_flips=max_flips)
        else:
            hdr = codec.decode_header(plan.run(heads).symbols, sf)
        status, hsym = hdr.status.view(R, C), hdr.nsym.view(R, C)
    else:
        status = hsym = torch.empty((R, C), dtype=torch.int32, device=dev)
    found, nsym = select_frames_device(cstarts, status, hsym, step, L, max_symbols, first, capacity)
    cap = found.starts.shape[1]
    max_bytes = codec.frame_capacity(sf, max_symbols)
    if R * cap == 0:
        none = {k: torch.empty(0, dtype=torch.int32, device=dev) for k in codec.FrameResult._FIELDS}
        frames = codec.FrameResult(payload=torch.empty((0, max_bytes), dtype=torch.uint8, device=dev), **none)
        return StreamPackets(found, nsym, _no_frames(max_symbols, dev), frames, ccount)
    at = torch.where(found.starts >= 0, found.starts + row0, found.starts).reshape(-1)
    length = (nsym.reshape(-1).to(torch.int64) + 2) * step
    slots = gather_frames_device(flat, at, length, cut)
    res = plan.run(slots)
    if soft:
        llr = plan.soft_bits(slots, res, reduced=(2, 8))
        frames = codec.decode_frame_soft(llr[:, 2:], sf, avail=nsym.reshape(-1), max_bytes=max_bytes,
                                         max_flips=max_flips)
        return StreamPackets(found, nsym, res, frames, ccount, llr)
    frames = codec.decode_frame(res.symbols, sf, avail=nsym.reshape(-1), max_bytes=max_bytes)
    return StreamPackets(found, nsym, res, frames, ccount)


def receive_frames_device(plan: DemodPlan, iq: torch.Tensor, max_symbols: int, hop: Optional[int] = None,
                          sync: int = 0x12, thresh_db: float = 0.0, first: Union[None, int, torch.Tensor] = None,
                          capacity: Optional[int] = None, cand_capacity: Optional[int] = None,
                          soft: bool = False, max_flips: int = 5) -> StreamPackets:
    """Receive self-describing frames (``codec.encode_frame``, ``LoRaMod.work_frame``) of any mix
    of lengths and coding rates from a [L] stream or [R, L] rows, with no frame length given and
    without the host: nothing is read back, nothing synchronises, every shape comes from host
    integers.  The steps: ``plan.scan``; ``find_candidates_device``; a gather of ``10 * step``
    samples per candidate; ``plan.run``; ``codec.decode_header``; ``select_frames_device`` (the
    greedy pass, over the candidates whose header is good, each frame as long as its header
    says); a gather of ``(2 + max_symbols) * step`` samples per slot, of which ``(2 + nsym) *
    step`` are the frame's and the rest zeros; ``plan.run``; ``codec.decode_frame`` with ``avail =
    nsym``.  The zeros make a slot's demodulation that of its frame alone (``plan.run`` on the
    frame zero-padded to the cut): the max-amplitude normalisation and the offset estimate see
    no neighbour's samples.

    ``max_symbols`` (>= 8): the longest frame accepted, in data symbols; a header that states
    more is passed over.  ``first`` and ``capacity`` as ``find_frames_device``'s; ``capacity``
    defaults to ``L // (10 * step)``, the most frames a row can hold - the second gather then
    holds ``R * capacity * (2 + max_symbols) * step`` samples, up to ``(2 + max_symbols) / 10``
    times the input, so a caller who knows their traffic passes a smaller one and watches
    ``found.count > capacity``.  ``cand_capacity`` defaults to ``ceil(L / (4 * step))`` (the first
    gather: ``R * cand_capacity * 10 * step`` samples, 2.5 times the input); ``candidates >
    cand_capacity`` tells that some were not probed.  The header is the guard against false
    candidates, so ``thresh_db`` may be negative here.

    Returns StreamPackets: ``found`` and ``nsym``, the DemodResult of ALL slots and their frame
    decode (``frames.status`` FRAME_OK / FRAME_CRC, ``frames.payload`` [R * capacity, max bytes of
    a max_symbols frame]); select with ``found.valid``.  A chunked caller overlaps chunks by
    ``(2 + max_symbols) * step - 1`` samples and carries ``found.end`` exactly as with
    ``receive_device``.  Limits, inherited from the finder: bw 125 kHz, ``hop`` dividing ``step``
    at least twice, and SF 7-12 (the header block).

    ``soft=True``: the same steps on soft decisions.  The header probe becomes ``plan.run``,
    ``plan.soft_bits(..., reduced=(2, 8))`` and ``codec.decode_header_soft``; the last step
    ``plan.run``, ``plan.soft_bits(..., reduced=(2, 8))`` over the slots and
    ``codec.decode_frame_soft`` on columns 2 onward with ``avail = nsym``.  Candidates, selection
    and gathers are unchanged, nothing synchronises, and ``llr`` of the result holds the slots'
    soft bits.  ``frames.errors`` then counts corrected codewords and ``frames.hdr_flips`` the
    header bits the decoder overruled; a header that needs more than ``max_flips`` (0 .. 40) of
    them is refused, which is what keeps noise from passing the soft header gate."""
    if not plan.dechirp:
        raise ValueError("receive_frames_device needs a plan with dechirp=True: the finder reads dechirped peaks")
    if not isinstance(iq, torch.Tensor) or iq.dim() not in (1, 2):
        raise ValueError("receive_frames_device takes one [L] stream or [R, L] rows")
    hop = plan.step // 4 if hop is None else int(hop)
    _geometry(hop, plan.sf, plan.osr, 8, sync, plan.bw)
    return _receive_frame_rows(plan, _check_iq(iq, plan.device), max_symbols, hop, sync, thresh_db, first, capacity,
                               cand_capacity, soft, max_flips)


def receive_wideband_frames_device(plan: DemodPlan, chan: "Channelizer", iq: torch.Tensor, max_symbols: int,
                                   hop: Optional[int] = None, sync: int = 0x12, thresh_db: float = 0.0,
                                   scale: Optional[float] = None, first: Union[None, int, torch.Tensor] = None,
                                   capacity: Optional[int] = None, cand_capacity: Optional[int] = None,
                                   soft: bool = False, max_flips: int = 5) -> StreamPackets:
    """``receive_frames_device`` for a wideband capture: ``chan.run`` on the [L] complex64 stream
    (or the raw [L, 2] integer stream, converted with ``scale``), then the same steps over the
    [C, Wc] channel rows - row r of the result is channel r, starts are in CHANNEL samples, and
    ``first`` ([C]) and the capacities count per channel with ``row_len = Wc``.  Channels may
    carry frames of different lengths at once.  ``soft`` and ``max_flips`` as
    ``receive_frames_device``'s.  No synchronisation."""
    if not plan.dechirp:
        raise ValueError("receive_wideband_frames_device needs a plan with dechirp=True: the finder reads "
                         "dechirped peaks")
    if not isinstance(iq, torch.Tensor) or iq.dim() != (2 if _is_raw(iq) else 1):
        raise ValueError("receive_wideband_frames_device takes one [L] stream (raw samples: [L, 2])")
    if chan.device != plan.device:
        raise ValueError(f"the channelizer is on {chan.device}, the plan is on {plan.device}")
    hop = plan.step // 4 if hop is None else int(hop)
    _geometry(hop, plan.sf, plan.osr, 8, sync, plan.bw)
    rows = chan.run(iq, scale=scale)  # [C, Wc]
    return _receive_frame_rows(plan, rows, max_symbols, hop, sync, thresh_db, first, capacity, cand_capacity, soft,
                               max_flips)


def _preamble_geometry(hop, sf, osr, acc_up, max_cfo_bins, bw):
    sf, osr, hop, acc_up = int(sf), int(osr) if osr else 1, int(hop), int(acc_up)
    if int(bw) != 125000:
        raise ValueError("the preamble finder is defined at bw 125000 only")
    if not 7 <= sf <= 12:
        raise ValueError("the preamble finder needs SF 7-12")
    N = 1 << sf
    step = N * osr
    if hop < 1 or step % hop != 0 or step // hop < 4:
        raise ValueError(f"hop must divide step = {step} at least four times (got {hop})")
    if not 2 <= acc_up <= 8:
        raise ValueError("preamble_acc must be in 2..8")
    max_cfo_bins = N // 4 - 1 if max_cfo_bins is None else int(max_cfo_bins)
    if not 0 <= max_cfo_bins <= N // 4 - 1:
        raise ValueError(f"max_cfo_bins must be in 0..{N // 4 - 1}")
    return N, step, step // hop, 9 * step // 4, max_cfo_bins


def preamble_threshold_db(sf: int) -> float:
    """The default of both thresholds of the preambled chain, from the measurement in DESIGN.md
    6p (profiles/stream/preamble_prob.json): -10 dB at SF7 and 3 dB lower per SF down to -22 dB -
    6 dB above the lowest value noise alone allows, which is where a frame's own data symbols stop
    crowding the candidate list.  SF 7, 9 and 12 were measured (-10, -16, -22); SF 8, 10 and 11 are
    interpolated."""
    return float(max(-10 - 3 * (int(sf) - 7), -22))


def find_preamble_device(up: DetectMetrics, dn: DetectMetrics, hop: int, sf: int, osr: int, acc_up: int,
                         thresh_up_db: float = 0.0, thresh_dn_db: float = 0.0, max_cfo_bins: Optional[int] = None,
                         row_len: Optional[int] = None, cand_capacity: Optional[int] = None, bw: int = 125000):
    """The preamble finder (lora_find_preamble_batch, one kernel; the rule is in this module's
    docstring): ``up`` is ``plan.scan_acc(rows, hop, acc_up)``, ``dn`` is ``plan.scan_acc(rows, hop,
    2, conj=True)`` of the same rows.  Returns ``(count, starts, cfo_bins)``: int32 [R] - the
    candidates listed, which may exceed the capacity - int64 [R, cand_capacity] starts (the first
    sync symbol; -1 beyond the count) and int32 [R, cand_capacity] carrier offsets in bins (0
    beyond the count).  ``row_len`` defaults to the span the down scan covers; ``cand_capacity`` to
    ``ceil(row_len / (4 * step))``; ``max_cfo_bins`` to ``N / 4 - 1``.  Nothing synchronises."""
    N, step, k, tail, max_cfo_bins = _preamble_geometry(hop, sf, osr, acc_up, max_cfo_bins, bw)
    hop, osr = int(hop), step // N
    upw, upa, upi, ups = _scan_rows(up, "find_preamble_device")
    dnw, dna, dni, dns = _scan_rows(dn, "find_preamble_device")
    R, Wu = upw.shape
    Wd = dnw.shape[1]
    if dnw.shape[0] != R or dnw.device != upw.device:
        raise ValueError("up and dn must be scans of the same rows on one device")
    if row_len is None:
        row_len = (Wd - 1) * hop + 2 * step if Wd else 0
    row_len = int(row_len)
    cap = _ceil_div(row_len, 4 * step) if cand_capacity is None else int(cand_capacity)
    if row_len < 0 or cap < 0:
        raise ValueError("row_len and cand_capacity must be >= 0")
    dev = upw.device
    count = torch.empty(R, dtype=torch.int32, device=dev)
    starts = torch.empty((R, cap), dtype=torch.int64, device=dev)
    cfo = torch.empty((R, cap), dtype=torch.int32, device=dev)
    if R:
        prm = _capi.PreambleParams(int(sf), osr, hop, int(acc_up), float(thresh_up_db), float(thresh_dn_db),
                                   max_cfo_bins, dev.index)
        ptr = lambda t, W: t.data_ptr() if W else None  # noqa: E731
        _capi.check(_capi.lib().lora_find_preamble_batch(
            _capi.C.byref(prm), ptr(upw, Wu), ptr(upa, Wu), ptr(upi, Wu), Wu, ups, ptr(dnw, Wd), ptr(dna, Wd),
            ptr(dni, Wd), Wd, dns, R, row_len, cap, starts.data_ptr() if cap else None,
            cfo.data_ptr() if cap else None, count.data_ptr(), _stream_handle(dev)))
    return count, starts, cfo


def select_preamble_device(cand_starts: torch.Tensor, cand_cfo: torch.Tensor, status: torch.Tensor,
                           nsym: torch.Tensor, step: int, row_len: int, max_symbols: int,
                           first: Union[None, int, torch.Tensor] = None, capacity: Optional[int] = None,
                           tail: Optional[int] = None) -> Tuple[FoundFrames, torch.Tensor, torch.Tensor]:
    """``select_frames_device`` for preambled frames (lora_select_preamble_batch, the same kernel):
    a frame ends at ``start + (2 + nsym) * step + tail`` (``tail`` defaults to ``9 * step // 4``), and
    each slot's ``cand_cfo`` (int32 [R, C]) is carried to the accepted slot - two candidates may share
    a start with different offsets, so the offset cannot be looked up afterwards.  ``capacity``
    defaults to ``row_len // (10 * step + tail)``.  Returns ``(found, nsym, cfo_bins)``; nothing
    synchronises."""
    for t, name, dt in ((cand_starts, "cand_starts", torch.int64), (cand_cfo, "cand_cfo", torch.int32),
                        (status, "status", torch.int32), (nsym, "nsym", torch.int32)):
        _require_cuda(t, name)
        if t.dtype != dt:
            raise TypeError(f"{name} must be {dt}, got {t.dtype}")
        if t.dim() != 2 or t.shape != cand_starts.shape or t.device != cand_starts.device or not t.is_contiguous():
            raise ValueError("cand_starts, cand_cfo, status and nsym must be contiguous [R, C] tensors on one device")
    R, C = cand_starts.shape
    dev = cand_starts.device
    step, row_len, max_symbols = int(step), int(row_len), int(max_symbols)
    tail = 9 * step // 4 if tail is None else int(tail)
    first_t = _find_first(first, R, dev)
    if first_t is not None and first_t.device != dev:
        raise ValueError(f"first must be on {dev}")
    capacity = row_len // (10 * step + tail) if capacity is None else int(capacity)
    if capacity < 0 or tail < 0:
        raise ValueError("capacity and tail must be >= 0")
    found = FoundFrames(count=torch.empty(R, dtype=torch.int32, device=dev),
                        starts=torch.empty((R, capacity), dtype=torch.int64, device=dev),
                        end=torch.empty(R, dtype=torch.int64, device=dev))
    out_nsym = torch.empty((R, capacity), dtype=torch.int32, device=dev)
    out_cfo = torch.zeros((R, capacity), dtype=torch.int32, device=dev)
    if R:
        if first_t is not None and not first_t.is_contiguous():
            first_t = first_t.contiguous()
        both = C > 0 and capacity > 0
        _capi.check(_capi.lib().lora_select_preamble_batch(
            cand_starts.data_ptr() if C else None, cand_cfo.data_ptr() if both else None,
            status.data_ptr() if C else None, nsym.data_ptr() if C else None, R, C,
            first_t.data_ptr() if first_t is not None else None, row_len, step, tail, max_symbols, capacity,
            found.starts.data_ptr() if capacity else None, out_cfo.data_ptr() if both else None,
            out_nsym.data_ptr() if capacity else None, found.count.data_ptr(), found.end.data_ptr(), dev.index,
            _stream_handle(dev)))
    return found, out_nsym, out_cfo


def _derotation_words(cfo_bins: torch.Tensor, step: int) -> torch.Tensor:
    """``floor(-c * 2**32 / step)`` in int64 on the device, wrapped into int32: the ``impair`` word
    that takes ``c`` bins (c cycles per symbol) off a slot."""
    w = torch.div(-cfo_bins.to(torch.int64) * (1 << 32), int(step), rounding_mode="floor") & 0xFFFFFFFF
    return torch.where(w >= 1 << 31, w - (1 << 32), w).to(torch.int32)


def _receive_preamble_rows(plan: DemodPlan, rows: torch.Tensor, max_symbols, preamble_acc, hop, sync, thresh_up_db,
                           thresh_dn_db, max_cfo_bins, first, capacity, cand_capacity, soft: bool = False,
                           max_flips: int = 5) -> StreamPackets:
    """The steps of ``receive_preamble_frames_device`` on [R, L] rows (checked by the caller)."""
    from . import codec

    sf, step, dev = plan.sf, plan.step, plan.device
    max_symbols = int(max_symbols)
    if max_symbols < 8:
        raise ValueError("max_symbols must be >= 8: a frame has at least its header's eight symbols")
    N, step, k, tail, max_cfo_bins = _preamble_geometry(hop, sf, plan.osr, preamble_acc, max_cfo_bins, plan.bw)
    thresh_up_db = preamble_threshold_db(sf) if thresh_up_db is None else float(thresh_up_db)
    thresh_dn_db = preamble_threshold_db(sf) if thresh_dn_db is None else float(thresh_dn_db)
    R, L = rows.shape
    up = plan.scan_acc(rows, hop, preamble_acc)
    dn = plan.scan_acc(rows, hop, 2, conj=True)
    ccount, cstarts, ccfo = find_preamble_device(up, dn, hop, sf, plan.osr, preamble_acc, thresh_up_db, thresh_dn_db,
                                                 max_cfo_bins, L, cand_capacity, plan.bw)
    C = cstarts.shape[1]
    rs = rows.stride(0) if R > 1 else L
    flat = rows.as_strided(((R - 1) * rs + L,), (1,)) if R else rows.reshape(-1)
    row0 = (torch.arange(R, device=dev) * rs)[:, None]

    def cut_slots(starts, cfo, data_len, cut):
        """[sync | data] of every slot - 2 * step samples at start, data_len at start + 2 * step +
        tail, zeros up to cut - with the slot's offset taken off (phase 0 at its first sample; the
        gather skips the delimiter, so the derotation's phase steps at the join, which the
        demodulator, non-coherent across symbols, does not see)."""
        at = torch.where(starts >= 0, starts + row0, starts).reshape(-1)
        buf = torch.empty((at.shape[0], cut + (cut & 1)), dtype=torch.complex64, device=dev)[:, :cut]
        gather_frames_device(flat, at, torch.full_like(at, 2 * step), 2 * step, out=buf[:, :2 * step])
        gather_frames_device(flat, torch.where(at >= 0, at + (2 * step + tail), at), data_len, cut - 2 * step,
                             out=buf[:, 2 * step:])
        return impair(buf, cfo=_derotation_words(cfo.reshape(-1), step), out=buf)

    if R * C:
        heads = cut_slots(cstarts, ccfo, torch.full((R * C,), 8 * step, dtype=torch.int64, device=dev), 10 * step)
        if soft:
            hdr = codec.decode_header_soft(plan.soft_bits(heads, plan.run(heads), reduced=(2, 8))[:, 2:], sf,
                                           max_flips=max_flips)
        else:
            hdr = codec.decode_header(plan.run(heads).symbols, sf)
        status, hsym = hdr.status.view(R, C), hdr.nsym.view(R, C)
    else:
        status = hsym = torch.empty((R, C), dtype=torch.int32, device=dev)
    found, nsym, cfo_bins = select_preamble_device(cstarts, ccfo, status, hsym, step, L, max_symbols, first, capacity,
                                                   tail)
    cap = found.starts.shape[1]
    max_bytes = codec.frame_capacity(sf, max_symbols)
    if R * cap == 0:
        none = {k_: torch.empty(0, dtype=torch.int32, device=dev) for k_ in codec.FrameResult._FIELDS}
        frames = codec.FrameResult(payload=torch.empty((0, max_bytes), dtype=torch.uint8, device=dev), **none)
        return StreamPackets(found, nsym, _no_frames(max_symbols, dev), frames, ccount, None, cfo_bins)
    slots = cut_slots(found.starts, cfo_bins, nsym.reshape(-1).to(torch.int64) * step, (2 + max_symbols) * step)
    res = plan.run(slots)
    if soft:
        llr = plan.soft_bits(slots, res, reduced=(2, 8))
        frames = codec.decode_frame_soft(llr[:, 2:], sf, avail=nsym.reshape(-1), max_bytes=max_bytes,
                                         max_flips=max_flips)
        return StreamPackets(found, nsym, res, frames, ccount, llr, cfo_bins)
    frames = codec.decode_frame(res.symbols, sf, avail=nsym.reshape(-1), max_bytes=max_bytes)
    return StreamPackets(found, nsym, res, frames, ccount, None, cfo_bins)


def receive_preamble_frames_device(plan: DemodPlan, iq: torch.Tensor, max_symbols: int, preamble_acc: int = 6,
                                   hop: Optional[int] = None, sync: int = 0x12,
                                   thresh_up_db: Optional[float] = None, thresh_dn_db: Optional[float] = None,
                                   max_cfo_bins: Optional[int] = None,
                                   first: Union[None, int, torch.Tensor] = None, capacity: Optional[int] = None,
                                   cand_capacity: Optional[int] = None, soft: bool = False,
                                   max_flips: int = 5) -> StreamPackets:
    """``receive_frames_device`` for preambled frames (``modulate_preamble``,
    ``LoRaMod.work_frame(preamble=...)``) under an integer carrier offset, without the host.  The
    steps: two accumulating scans (``plan.scan_acc(rows, hop, preamble_acc)`` and ``plan.scan_acc(rows,
    hop, 2, conj=True)``); ``find_preamble_device``; the header probe - two gathers into one buffer,
    ``2 * step`` samples at each start and ``8 * step`` at ``start + 2 * step + tail``, empty slots
    staying negative, then ``impair(buf, cfo=words, out=buf)`` with ``words = floor(-c * 2**32 /
    step)`` wrapped into int32, one per slot - ``plan.run``; ``codec.decode_header`` (or its soft
    form); ``select_preamble_device`` with the tail; the same two gathers at ``(2 + max_symbols) *
    step`` with ``nsym * step`` of data; derotation, ``plan.run``, ``codec.decode_frame`` (or soft).
    Nothing is read back and nothing synchronises.

    ``thresh_up_db`` and ``thresh_dn_db`` default to ``preamble_threshold_db(sf)``, the measured choice
    (-10 dB at SF7 to -22 dB at SF 11-12): lower values find no more frames at the default
    ``cand_capacity``, because a frame's own data symbols then fill the candidate list.
    ``preamble_acc`` (2..8) must not exceed the transmitter's preamble length; ``hop`` defaults to
    ``step // 4`` and must divide ``step`` at least four times; ``max_cfo_bins`` defaults to ``N / 4
    - 1``.  Returns StreamPackets with ``cfo_bins`` [R, capacity], each frame's offset in bins; the
    residual fraction of a bin stays with the demodulator's own estimate (``result.cfo``).  The
    ``sync`` word is the demodulator's to report (``result.sync``): the preamble finder does not
    use it.  Limits: bw 125 kHz, SF 7-12, this project's own frame layout, one workgroup per row
    in the finder kernels."""
    if not plan.dechirp:
        raise ValueError("receive_preamble_frames_device needs a plan with dechirp=True: the finder reads "
                         "dechirped peaks")
    if not isinstance(iq, torch.Tensor) or iq.dim() not in (1, 2):
        raise ValueError("receive_preamble_frames_device takes one [L] stream or [R, L] rows")
    hop = plan.step // 4 if hop is None else int(hop)
    return _receive_preamble_rows(plan, _check_iq(iq, plan.device), max_symbols, preamble_acc, hop, sync, thresh_up_db,
                                  thresh_dn_db, max_cfo_bins, first, capacity, cand_capacity, soft, max_flips)


def receive_wideband_preamble_frames_device(plan: DemodPlan, chan: "Channelizer", iq: torch.Tensor, max_symbols: int,
                                            preamble_acc: int = 6, hop: Optional[int] = None, sync: int = 0x12,
                                            thresh_up_db: Optional[float] = None,
                                            thresh_dn_db: Optional[float] = None,
                                            max_cfo_bins: Optional[int] = None, scale: Optional[float] = None,
                                            first: Union[None, int, torch.Tensor] = None,
                                            capacity: Optional[int] = None, cand_capacity: Optional[int] = None,
                                            soft: bool = False, max_flips: int = 5) -> StreamPackets:
    """``receive_preamble_frames_device`` for a wideband capture: ``chan.run`` on the [L] complex64
    stream (or the raw [L, 2] integer stream, converted with ``scale``), then the same steps over
    the [C, Wc] channel rows, as ``receive_wideband_frames_device``.  No synchronisation."""
    if not plan.dechirp:
        raise ValueError("receive_wideband_preamble_frames_device needs a plan with dechirp=True: the finder reads "
                         "dechirped peaks")
    if not isinstance(iq, torch.Tensor) or iq.dim() != (2 if _is_raw(iq) else 1):
        raise ValueError("receive_wideband_preamble_frames_device takes one [L] stream (raw samples: [L, 2])")
    if chan.device != plan.device:
        raise ValueError(f"the channelizer is on {chan.device}, the plan is on {plan.device}")
    hop = plan.step // 4 if hop is None else int(hop)
    rows = chan.run(iq, scale=scale)  # [C, Wc]
    return _receive_preamble_rows(plan, rows, max_symbols, preamble_acc, hop, sync, thresh_up_db, thresh_dn_db,
                                  max_cfo_bins, first, capacity, cand_capacity, soft, max_flips)


def gather_frames_device(iq: torch.Tensor, at: torch.Tensor, length: torch.Tensor, cut: int,
                         out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Cut frames of different lengths out of a stream, on the device (lora_gather_frames_batch,
    one kernel): ``out[s, t] = flat[at[s] + t]`` for ``t < length[s]`` and 0 up to ``cut``.

    ``iq`` is a [L] complex64 CUDA stream, or [R, L] rows as ``scan`` takes them, read as the one
    flat stream in which sample t of row r is ``r * iq.stride(0) + t``.  ``at`` and ``length``
    are int64 [K] tensors on its device - the finder's starts and ``(2 + nsym) * step``, never
    read on the host.  A slot with ``at < 0`` (the finder's empty slot) is all zeros; ``length``
    is clamped to ``0..cut`` and to the stream's end, so nothing at or beyond ``at + length`` is
    read.  The zeros after a frame make its demodulation a function of the frame alone: it
    equals ``plan.run`` on the frame zero-padded to ``cut`` whatever follows it in the stream.

    Returns complex64 [K, cut]; its rows are 16-byte aligned, so with an odd ``cut`` they are
    ``cut + 1`` samples apart (``plan.run`` takes such rows).  ``out``: a tensor of that layout to
    write into.  Nothing synchronises."""
    iq = _check_iq(iq, iq.device if isinstance(iq, torch.Tensor) else None)
    dev = iq.device
    cut = int(cut)
    if cut < 0:
        raise ValueError("cut must be >= 0")
    for t, name in ((at, "at"), (length, "length")):
        _require_cuda(t, name)
        if t.dtype != torch.int64:
            raise TypeError(f"{name} must be an int64 tensor, got {t.dtype}")
        if t.dim() != 1 or t.device != dev:
            raise ValueError(f"{name} must be a 1-D tensor on {dev}")
    K = at.shape[0]
    if length.shape[0] != K:
        raise ValueError("at and length must have one entry per slot")
    at, length = at.contiguous(), length.contiguous()
    R, L = iq.shape
    total = (R - 1) * iq.stride(0) + L if R > 1 else L * min(R, 1)
    pitch = cut + (cut & 1)
    if out is None:
        out = torch.empty((K, pitch), dtype=torch.complex64, device=dev)[:, :cut]
    else:
        _require_cuda(out, "out")
        if (out.dtype != torch.complex64 or out.device != dev or tuple(out.shape) != (K, cut)
                or (cut > 1 and out.stride(1) != 1) or (K > 1 and (out.stride(0) < cut or out.stride(0) & 1))
                or out.data_ptr() & 15):
            raise ValueError(f"out must be a complex64 [{K}, {cut}] tensor on {dev} with 16-byte aligned rows")
    if K and cut:
        _capi.check(_capi.lib().lora_gather_frames_batch(
            iq.data_ptr() if total else None, total, at.data_ptr(), length.data_ptr(), K, cut, out.data_ptr(),
            out.stride(0) if K > 1 else pitch, dev.index, _stream_handle(dev)))
    return out


# raw output dtypes of the synthesis bank: the default inv_scale (exact in fp32)
_INV_SCALE = {torch.int16: 32768.0, torch.int8: 128.0, torch.uint8: 127.5}


class Synthesizer:
    """A synthesis bank on the GPU, the inverse of ``Channelizer``: ``C = len(steps)`` channel
    streams in, one wideband stream at ``interp`` times their rate out.  Channel c is multiplied
    by ``gains[c]`` (default 1), interpolated by ``interp`` with the real ``taps`` - a prototype
    low-pass at the OUTPUT rate, ``lowpass_taps(ntaps, 0.5 / interp, gain=interp)`` - mixed up to
    ``steps[c] / period`` cycles per output sample above the centre, and the channels are summed.
    One kernel (lora_synthesize_batch) writes every wideband sample once, as complex64 or, with
    ``dtype``, as the raw integer samples a radio takes (lora_synthesize_raw_batch: ``int16`` for a
    USRP or Pluto, ``int8`` for a HackRF, ``uint8``).  The arithmetic is defined exactly in
    include/lora_mi355x.h (the definition is this library's own: the reference has no
    synthesiser), so a host restatement reproduces every bit.

    Limits: ``interp`` 1..64, 1..512 taps, ``period`` 1..4096, 1..32 channels; channel centres
    are multiples of ``fs / period``.  Only an integer ``interp`` is covered: a rational up-rate
    (interp / decim) is not.  Nothing is claimed about the spectrum beyond what the taps do: no
    spectral-mask or adjacent-channel figure, and nothing of a DAC or a front end.

    The taps and the oscillator table - ``exp(+2 pi i m / period)``, the conjugate of
    ``nco_table(period)`` - are kept on the device.  ``delay``: channel sample m is centred on
    output ``m * interp + delay``, ``delay = (ntaps - 1) / 2 - (P - 1) * interp`` with ``P =
    ceil(ntaps / interp)`` (it is negative when the first "valid" output lies past the centre of
    channel sample 0)."""

    def __init__(self, interp: int, taps, period: int, steps, gains=None, device=None):
        self.interp, self.period = int(interp), int(period)
        h = np.ascontiguousarray(taps, np.float32)
        self.steps = [int(k) for k in steps]
        if not 1 <= self.interp <= 64:
            raise ValueError("interp must be in 1..64")
        if h.ndim != 1 or not 1 <= h.shape[0] <= 512:
            raise ValueError("taps must be 1..512 real values")
        if not 1 <= self.period <= 4096:
            raise ValueError("period must be in 1..4096")
        if not 1 <= len(self.steps) <= 32 or any(abs(k) >= 1 << 31 for k in self.steps):
            raise ValueError("steps must be 1..32 ints")
        self.ntaps, self.channels = int(h.shape[0]), len(self.steps)
        g = np.ones(self.channels, np.float32) if gains is None else np.ascontiguousarray(gains, np.float32)
        if g.shape != (self.channels,):
            raise ValueError("gains must be one real value per channel")
        self.gains = [float(v) for v in g]
        self.P = -(-self.ntaps // self.interp)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise TypeError("Synthesizer runs on a CUDA (HIP) device; there is no CPU fallback")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._lib = _capi.lib()
        self._steps = (_capi.C.c_int32 * self.channels)(*self.steps)
        self._gains = (_capi.C.c_float * self.channels)(*self.gains)
        self.taps = torch.from_numpy(h.copy()).to(self.device)
        self.nco = torch.from_numpy(np.conj(nco_table(self.period))).to(self.device)

    @property
    def delay(self) -> float:
        return (self.ntaps - 1) / 2 - (self.P - 1) * self.interp

    def _outputs(self, chan_len: int) -> int:
        return 0 if chan_len < self.P else (chan_len - self.P + 1) * self.interp

    def outputs(self, chan_len: int) -> int:
        """Wideband samples for channel streams of ``chan_len`` samples: ``0 if chan_len < P else
        (chan_len - P + 1) * interp`` (lora_synthesize_outputs)."""
        return _capi.check(self._lib.lora_synthesize_outputs(int(chan_len), self.ntaps, self.interp))

    def run(self, chans: torch.Tensor, first_sample: int = 0, out: Optional[torch.Tensor] = None, dtype=None,
            inv_scale: Optional[float] = None) -> torch.Tensor:
        """Synthesize [C, Lc] complex64 CUDA channel streams into a [W] complex64 wideband stream,
        or [R, C, Lc] into [R, W]; ``W = outputs(Lc)``.  The streams have unit sample stride and
        are any equal number of samples >= Lc apart (rows ``C`` times that), so a [.., :Lc] view
        of a larger tensor is accepted.  With ``dtype`` ``torch.int16``, ``torch.int8`` or
        ``torch.uint8`` the result is raw samples [W, 2] or [R, W, 2] (I, Q), each component
        ``clamp(rint(y * inv_scale (+ 127.5 for uint8)))`` in fp32 with ties to even and NaN stored
        as the format's zero; ``inv_scale`` defaults to 32768, 128 or 127.5 and is rounded to fp32
        (``inv_scale`` without ``dtype`` is a ``ValueError``).  That is ``iq_io.quantize`` of the
        complex64 result wherever its division by ``scale`` and this product round alike - the
        power-of-two scales, i.e. the ``int16`` and ``int8`` defaults - in one kernel and with no
        complex64 copy.  ``first_sample`` (>= 0) is the index of output 0 in the transmitted
        recording, which keeps the oscillators' phase continuous across chunks: a chunk whose
        streams overlap its predecessor's by ``P - 1`` samples and whose ``first_sample`` is
        advanced by the predecessor's ``W`` continues its outputs.
        ``out``: a tensor of the result's dtype to write into, [>= W] (or [R, >= W]; raw: with a
        trailing 2), unit stride within a row and rows that do not overlap; any slice ``buf[k:]``
        of a transmit buffer will do, the kernel needs no alignment beyond one sample.  Its
        columns from W on are left alone and the [.., :W] view is returned.  One kernel on the
        current stream, nothing allocated besides the output, so the call can be captured in a
        HIP graph."""
        if dtype is None:
            if inv_scale is not None:
                raise ValueError("inv_scale belongs to a raw integer dtype; a complex64 output has none")
            odt = torch.complex64
        else:
            if dtype not in _INV_SCALE:
                raise TypeError(f"raw samples are int16 (cs16), int8 (cs8) or uint8 (cu8), not {dtype}")
            odt = dtype
            inv_scale = float(np.float32(_INV_SCALE[dtype] if inv_scale is None else inv_scale))
        raw = dtype is not None
        _require_cuda(chans, "chans")
        if chans.device != self.device:
            raise ValueError(f"chans is on {chans.device}, the synthesizer is on {self.device}")
        if chans.dtype != torch.complex64:
            raise TypeError("chans must be complex64")
        if chans.dim() not in (2, 3) or chans.shape[-2] != self.channels:
            raise ValueError(f"chans must be [{self.channels}, Lc] or [R, {self.channels}, Lc]")
        one = chans.dim() == 2
        if one:
            chans = chans.unsqueeze(0)
        R, C, Lc = chans.shape
        in_stride = chans.stride(1) if C > 1 else (chans.stride(0) // C if R > 1 else Lc)
        if ((Lc > 1 and chans.stride(2) != 1) or (R * C > 1 and in_stride < Lc)
                or (R > 1 and chans.stride(0) != C * in_stride)):
            raise ValueError("chans must have unit sample stride, streams an equal number of samples >= Lc apart "
                             "and rows C times that")
        first_sample = int(first_sample)
        if first_sample < 0:
            raise ValueError("first_sample must be >= 0")
        W = self._outputs(Lc)
        tail = (2,) if raw else ()
        if out is None:
            out = torch.empty(((W,) if one else (R, W)) + tail, dtype=odt, device=self.device)
        else:
            _require_cuda(out, "out")
            if out.dtype != odt:
                raise TypeError(f"out must be {odt}")
            lead = () if one else (R,)
            nd = len(lead) + 1 + len(tail)
            ok = (out.device == self.device and out.dim() == nd and tuple(out.shape[:len(lead)]) == lead
                  and out.shape[len(lead)] >= W and (not raw or (out.shape[-1] == 2 and out.stride(-1) == 1)))
            per = 2 if raw else 1  # elements per sample
            if ok and out.shape[len(lead)] > 1:
                ok = out.stride(len(lead)) == per
            if ok and R > 1 and not one:
                ok = out.stride(0) % per == 0 and out.stride(0) >= per * W
            if not ok:
                raise ValueError(f"out must be a {odt} {list(lead) + ['>=%d' % W] + list(tail)} tensor on "
                                 f"{self.device} with unit stride within a row and rows that do not overlap")
        view = out[:W] if one else out[:, :W]
        if R == 0 or W == 0:
            return view  # nothing to launch (and an empty tensor has no address to pass)
        out_stride = (out.stride(0) // (2 if raw else 1)) if (not one and R > 1) else out.shape[0 if one else 1]
        head = (chans.data_ptr(), R, Lc, in_stride, first_sample, self.taps.data_ptr(), self.ntaps, self.interp,
                self.nco.data_ptr(), self.period, self._steps, self._gains, C, out.data_ptr())
        tail_args = (out_stride, self.device.index, _stream_handle(self.device))
        if raw:
            got = self._lib.lora_synthesize_raw_batch(*head, _RAW[dtype][0], inv_scale, *tail_args)
        else:
            got = self._lib.lora_synthesize_batch(*head, *tail_args)
        got = _capi.check(got)
        assert got == W, (got, W)
        return view


def transmit_wideband(synth: Synthesizer, frames: torch.Tensor, channel, starts, chan_len: int,
                      first_sample: int = 0, out: Optional[torch.Tensor] = None, dtype=None,
                      inv_scale: Optional[float] = None) -> torch.Tensor:
    """The inverse of ``receive_wideband``: put K frames into the channels of one wideband stream.
    ``frames`` is a [K, frame_len] complex64 CUDA tensor (``LoRaMod.work``'s); frame i goes to
    samples ``starts[i] .. starts[i] + frame_len - 1`` of channel ``channel[i]`` (host ints, in
    CHANNEL samples) of a zeroed [C, chan_len] tensor - one torch index assignment - which
    ``synth.run`` then turns into the wideband stream: [W] complex64, or [W, 2] raw samples with
    ``dtype``; ``first_sample``, ``out``, ``dtype`` and ``inv_scale`` are ``Synthesizer.run``'s.
    Channel sample m is centred on output ``m * synth.interp + synth.delay``.  A frame outside
    its channel's ``chan_len`` samples, a channel outside 0 .. C-1 or two frames that overlap in
    one channel are a ``ValueError``."""
    _require_cuda(frames, "frames")
    if frames.dtype != torch.complex64 or frames.dim() != 2:
        raise ValueError("frames must be a [K, frame_len] complex64 tensor")
    if frames.device != synth.device:
        raise ValueError(f"frames is on {frames.device}, the synthesizer is on {synth.device}")
    K, frame_len = frames.shape
    chan_len = int(chan_len)
    ch = np.asarray(channel.cpu() if isinstance(channel, torch.Tensor) else channel, np.int64).reshape(-1)
    st = np.asarray(starts.cpu() if isinstance(starts, torch.Tensor) else starts, np.int64).reshape(-1)
    if len(ch) != K or len(st) != K:
        raise ValueError("channel and starts must have one entry per frame")
    if K and (ch.min() < 0 or ch.max() >= synth.channels):
        raise ValueError(f"channel must be in 0..{synth.channels - 1}")
    if K and (st.min() < 0 or st.max() + frame_len > chan_len):
        raise ValueError("every frame must lie inside its channel's chan_len samples")
    order = np.lexsort((st, ch))
    for i, j in zip(order[:-1], order[1:]):
        if ch[i] == ch[j] and st[j] < st[i] + frame_len:
            raise ValueError(f"frames {int(i)} and {int(j)} overlap in channel {int(ch[i])}")
    chans = torch.zeros((synth.channels, chan_len), dtype=torch.complex64, device=synth.device)
    if K and frame_len:
        base = torch.from_numpy(ch * chan_len + st).to(synth.device)
        idx = base[:, None] + torch.arange(frame_len, device=synth.device)
        chans.view(-1)[idx] = frames
    return synth.run(chans, first_sample, out, dtype, inv_scale)


def cfo_word(cycles_per_sample: float) -> int:
    """A carrier offset in cycles per sample as ``impair``'s 32-bit frequency control word:
    ``round(cycles_per_sample * 2**32)`` to nearest, wrapped into int32 (one step is fs / 2**32;
    0.5 and -0.5 cycles per sample are the same word, -2**31)."""
    w = int(round(float(cycles_per_sample) * 4294967296.0)) & 0xFFFFFFFF
    return w - (1 << 32) if w >= 1 << 31 else w


def noise_sigma(snr_db: float, amplitude: float = 1.0) -> float:
    """The per-component noise deviation that puts a signal of ``amplitude`` at ``snr_db`` dB:
    ``amplitude * 10**(-snr_db / 20) / sqrt(2)`` (``awgn.sweep_chain``'s convention: the complex
    noise power is ``2 * sigma**2``)."""
    return float(amplitude) * 10.0 ** (-float(snr_db) / 20.0) / float(np.sqrt(2.0))


def _row_values(v, R: int, dev: torch.device, name: str, words: bool) -> Optional[torch.Tensor]:
    """A per-row parameter as the kernel takes it: None, or a contiguous [R] tensor on ``dev`` -
    float32, or int32 words when ``words`` (a float value is in cycles and becomes
    ``round(v * 2**32)`` wrapped into int32, an int32 tensor is taken as words).  Tensor
    arithmetic only: nothing is read back."""
    if v is None:
        return None
    if isinstance(v, torch.Tensor):
        if v.dim() > 1 or (v.dim() == 1 and v.shape[0] not in (1, R)):
            raise ValueError(f"{name} must be a scalar or one value per row ([{R}])")
        if v.device != dev:
            raise ValueError(f"{name} is on {v.device}, the samples are on {dev}")
        t = v.reshape(-1).expand(R) if v.numel() == 1 else v
        if words and t.dtype == torch.int32:
            return t.contiguous()
        if not words:
            return t.to(torch.float32).contiguous()
        w = torch.round(t.to(torch.float64) * 4294967296.0).to(torch.int64) & 0xFFFFFFFF
        return torch.where(w >= 1 << 31, w - (1 << 32), w).to(torch.int32).contiguous()
    if words:
        return torch.full((R,), cfo_word(v), dtype=torch.int32, device=dev)
    return torch.full((R,), float(np.float32(v)), dtype=torch.float32, device=dev)


def impair(iq: Optional[torch.Tensor], *, sigma=None, snr_db=None, amplitude=1.0, cfo=None, phase=None, gain=None,
           seed: int = 0, first_sample: int = 0, first_row: int = 0, out: Optional[torch.Tensor] = None, dtype=None,
           scale: Optional[float] = None, rows: Optional[int] = None, length: Optional[int] = None,
           device=None) -> torch.Tensor:
    """The channel between a transmitter and a receiver, one kernel that reads the samples once and
    writes them once (lora_impair_batch, lora_impair_raw_batch; the exact arithmetic is in
    include/lora_mi355x.h and is this project's own): per row a ``gain``, a carrier offset ``cfo``
    in cycles per sample with a starting ``phase`` in cycles (both through ``cfo_word``: a 32-bit
    phase accumulator, continuous across chunks by construction), and white Gaussian noise of
    deviation ``sigma`` per component - or ``snr_db`` for a signal of ``amplitude``
    (``noise_sigma``); the two are mutually exclusive.  Each is a scalar or a per-row tensor on
    the samples' device (an int32 tensor for ``cfo`` or ``phase`` is taken as words), and a stage
    whose parameter is None is not performed at all.

    ``iq``: [L] or [R, L] complex64 CUDA samples (unit sample stride, rows that do not overlap;
    any slice will do, the kernel needs no alignment beyond one sample), or None for noise-only
    rows of ``rows`` x ``length`` (``rows=None``: one [length] row) on ``device``.  The noise of
    sample t of row r is a function of ``(seed, first_row + r, first_sample + t)`` alone (Philox
    4x32-10 and Box-Muller, each component N(0, sigma^2) truncated at 5.77 sigma), so a
    recording impaired in chunks, or by several ranks a few rows each, is bit for bit the
    recording impaired at once, and a host restatement reproduces every bit.

    ``out``: a tensor to write into, of the result's shape and dtype; ``out=iq`` runs in place.
    ``dtype`` ``torch.int16``, ``torch.int8`` or ``torch.uint8`` gives raw samples [.., L, 2]
    stored by ``Synthesizer.run``'s rule, ``scale`` being its ``inv_scale`` (default 32768, 128,
    127.5; ``scale`` without ``dtype`` is a ``ValueError``).  Returns the result.  One kernel on
    the current stream; it never synchronises and never reads device memory on the host.

    A fractional delay, multipath, a clock offset and frequency drift are ``propagate``'s, which
    goes in front.  Not covered: DC offset, IQ imbalance or any other front-end effect, and
    time-varying path gains; an integer delay is a slice."""
    if sigma is not None and snr_db is not None:
        raise ValueError("sigma and snr_db are mutually exclusive")
    if dtype is None:
        if scale is not None:
            raise ValueError("scale belongs to a raw integer dtype; a complex64 output has none")
        odt = torch.complex64
    else:
        if dtype not in _INV_SCALE:
            raise TypeError(f"raw samples are int16 (cs16), int8 (cs8) or uint8 (cu8), not {dtype}")
        odt = dtype
        scale = float(np.float32(_INV_SCALE[dtype] if scale is None else scale))
    raw = dtype is not None
    if iq is None:
        if length is None:
            raise ValueError("noise-only rows (iq=None) need length, and rows for more than one")
        one = rows is None
        R, L = (1 if one else int(rows)), int(length)
        if R < 0 or L < 0:
            raise ValueError("rows and length must be >= 0")
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise TypeError("impair runs on a CUDA (HIP) device; there is no CPU fallback")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if sigma is None and snr_db is None:
            raise ValueError("noise-only rows need sigma or snr_db")
        if cfo is not None or phase is not None or gain is not None:
            raise ValueError("noise-only rows take no cfo, phase or gain")
        in_ptr, in_stride = None, L
    else:
        if rows is not None or length is not None or device is not None:
            raise ValueError("rows, length and device belong to noise-only rows (iq=None)")
        _require_cuda(iq, "iq")
        one = iq.dim() == 1
        dev = iq.device
        x = _check_iq(iq, dev)
        R, L = x.shape
        in_ptr, in_stride = x.data_ptr(), (x.stride(0) if R > 1 else L)
    first_sample, first_row, seed = int(first_sample), int(first_row), int(seed)
    if first_sample < 0 or first_row < 0:
        raise ValueError("first_sample and first_row must be >= 0")
    if not 0 <= seed < 1 << 64:
        raise ValueError("seed must be in 0 .. 2**64 - 1")
    if snr_db is not None:
        if isinstance(snr_db, torch.Tensor) or isinstance(amplitude, torch.Tensor):
            db = snr_db if isinstance(snr_db, torch.Tensor) else torch.tensor(float(snr_db), device=dev)
            sigma = amplitude * torch.pow(10.0, -db.to(torch.float64) / 20.0) / float(np.sqrt(2.0))
        else:
            sigma = noise_sigma(snr_db, amplitude)
    g_t = _row_values(gain, R, dev, "gain", False)
    s_t = _row_values(sigma, R, dev, "sigma", False)
    f_t = _row_values(cfo, R, dev, "cfo", True)
    p_t = _row_values(phase, R, dev, "phase", True)
    if g_t is None and s_t is None and f_t is None and p_t is None:
        raise ValueError("nothing to do: give at least one of sigma / snr_db, cfo, phase, gain")
    lead = () if one else (R,)
    tail = (2,) if raw else ()
    per = 2 if raw else 1  # elements per sample
    if out is None:
        out = torch.empty(lead + (L,) + tail, dtype=odt, device=dev)
    else:
        _require_cuda(out, "out")
        if out.dtype != odt:
            raise TypeError(f"out must be {odt}")
        ok = out.device == dev and tuple(out.shape) == lead + (L,) + tail and (not raw or out.stride(-1) == 1)
        if ok and L > 1:
            ok = out.stride(len(lead)) == per
        if ok and R > 1 and not one:
            ok = out.stride(0) % per == 0 and out.stride(0) >= per * L
        if not ok:
            raise ValueError(f"out must be a {odt} {list(lead + (L,) + tail)} tensor on {dev} with unit stride "
                             "within a row and rows that do not overlap")
    if R == 0 or L == 0:
        return out  # nothing to launch (and an empty tensor has no address to pass)
    out_stride = (out.stride(0) // per) if (not one and R > 1) else L
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    head = (in_ptr, R, L, in_stride, first_sample, first_row, seed, ptr(g_t), ptr(f_t), ptr(p_t), ptr(s_t),
            out.data_ptr())
    tail_args = (out_stride, dev.index, _stream_handle(dev))
    lib = _capi.lib()
    if raw:
        got = lib.lora_impair_raw_batch(*head, _RAW[dtype][0], scale, *tail_args)
    else:
        got = lib.lora_impair_batch(*head, *tail_args)
    got = _capi.check(got)
    assert got == L, (got, L)
    return out


# ---- propagation: multipath, fractional delay, clock offset, drift (lora_propagate_batch) -------

# The Kaiser beta of the default table: the value with the smallest worst-case response error over
# all 256 phases and |f| <= 0.4 cycles per sample at 16 taps (DESIGN.md section 6q has the sweep)
FRACDELAY_BETA = 5.05

_MAX_DELAY_WORD = 1 << 47
_MAX_SFO_WORD = 1 << 20
_default_tables: dict = {}


def fracdelay_table(taps: int = 16, beta: float = FRACDELAY_BETA) -> np.ndarray:
    """``propagate``'s fractional-delay interpolator: [256, taps] float32, row ``ph`` a filter that
    delays by ``taps/2 - 1 + ph/256`` samples.  A Kaiser-windowed sinc evaluated in float64:
    ``u = t - (taps/2 - 1) - ph/256``, ``h = sinc(u) * I0(beta * sqrt(1 - (u / (taps/2))**2)) /
    I0(beta)`` and zero where ``|u| > taps/2``; every row is normalised to sum 1 in float64 and then
    rounded to fp32; row 0 is the exact unit impulse at ``t = taps/2 - 1``, so a whole-sample delay
    is a copy.  ``taps`` is even, 2..32."""
    taps = int(taps)
    if taps < 2 or taps > 32 or taps % 2:
        raise ValueError("taps must be even and in 2..32")
    half = taps // 2
    u = np.arange(taps, dtype=np.float64)[None, :] - (half - 1) - np.arange(256, dtype=np.float64)[:, None] / 256.0
    z = 1.0 - (u / half) ** 2
    h = np.where(z >= 0.0, np.sinc(u) * np.i0(float(beta) * np.sqrt(np.maximum(z, 0.0))) / np.i0(float(beta)), 0.0)
    h /= h.sum(axis=1, keepdims=True)
    table = h.astype(np.float32)
    table[0] = 0.0
    table[0, half - 1] = 1.0
    return table


def delay_word(samples: float) -> int:
    """A delay in samples as ``propagate``'s word: ``round(samples * 2**32)``, to nearest with ties
    to even (one step is 2**-32 sample).  ``|word| > 2**47`` (32768 samples) is a ``ValueError``."""
    w = int(round(float(samples) * 4294967296.0))
    if abs(w) > _MAX_DELAY_WORD:
        raise ValueError("a delay is at most 2**15 samples either way")
    return w


def sfo_word(ppm: float) -> int:
    """A sample-clock offset in parts per million as ``propagate``'s word: ``round(ppm * 1e-6 *
    2**32)``, to nearest with ties to even (one step is 2**-32 sample per sample).  ``|word| >
    2**20`` (about 244 ppm) is a ``ValueError``."""
    w = int(round(float(ppm) * 1e-6 * 4294967296.0))
    if abs(w) > _MAX_SFO_WORD:
        raise ValueError("a sample-clock offset is at most 2**20 words (about 244 ppm) either way")
    return w


def _wrap64(w: int) -> int:
    w &= (1 << 64) - 1
    return w - (1 << 64) if w >= 1 << 63 else w


def cfo_word64(cycles_per_sample: float) -> int:
    """A carrier offset in cycles per sample as ``propagate``'s 64-bit frequency control word:
    ``round(cycles_per_sample * 2**64)`` to nearest, wrapped into int64 (one step is fs / 2**64;
    0.5 and -0.5 are the same word, -2**63).  ``cfo_word(c) << 32`` is ``impair``'s offset."""
    c = float(cycles_per_sample)
    if not np.isfinite(c):
        raise ValueError("a carrier offset must be finite")
    return _wrap64(int(round(c * 18446744073709551616.0)))


def drift_word(hz_per_s: float, fs: float) -> int:
    """A carrier drift in Hz per second at the sample rate ``fs`` (Hz) as ``propagate``'s word:
    ``round(hz_per_s / fs**2 * 2**64)`` to nearest (one step is fs / 2**64 per sample).  A drift
    whose word does not fit int64 (half a cycle per sample, per sample) is a ``ValueError``."""
    fs = float(fs)
    if not fs > 0.0 or not np.isfinite(float(hz_per_s)):
        raise ValueError("fs must be positive and the drift finite")
    w = int(round(float(hz_per_s) / (fs * fs) * 18446744073709551616.0))
    if not -(1 << 63) <= w < 1 << 63:
        raise ValueError("the drift does not fit the 64-bit word")
    return w


def _path_array(v, R: int, name: str):
    """A per-path host value as a [1 or R, P] array: a scalar, [P] or [R, P]."""
    a = np.asarray(v)
    if a.ndim == 0:
        a = a.reshape(1, 1)
    elif a.ndim == 1:
        a = a.reshape(1, -1)
    if a.ndim != 2 or a.shape[0] not in (1, R) or a.shape[1] < 1:
        raise ValueError(f"{name} must be a scalar, one value per path ([P]) or per row and path ([{R}, P])")
    return a


def _path_delay(v, R: int, dev: torch.device) -> torch.Tensor:
    """``delay`` as [1 or R, P] int64 words on ``dev``: host values go through ``delay_word``, a
    float tensor is rounded on the device, an int64 tensor is taken as words (a tensor's range is
    its owner's contract: nothing is read back)."""
    if isinstance(v, torch.Tensor):
        if v.device != dev:
            raise ValueError(f"delay is on {v.device}, the samples are on {dev}")
        t = v.reshape(1, 1) if v.dim() == 0 else v.reshape(1, -1) if v.dim() == 1 else v
        if t.dim() != 2 or t.shape[0] not in (1, R) or t.shape[1] < 1:
            raise ValueError(f"delay must be a scalar, [P] or [{R}, P]")
        return t if t.dtype == torch.int64 else torch.round(t.to(torch.float64) * 4294967296.0).to(torch.int64)
    a = _path_array(v, R, "delay")
    w = np.array([[delay_word(x) for x in row] for row in a.tolist()], np.int64)
    return torch.from_numpy(w).to(dev)


def _path_gain(v, R: int, dev: torch.device) -> torch.Tensor:
    """``gain`` as [1 or R, P, 2] float32 (re, im) on ``dev``."""
    if isinstance(v, torch.Tensor):
        if v.device != dev:
            raise ValueError(f"gain is on {v.device}, the samples are on {dev}")
        t = v.reshape(1, 1) if v.dim() == 0 else v.reshape(1, -1) if v.dim() == 1 else v
        if t.dim() != 2 or t.shape[0] not in (1, R) or t.shape[1] < 1:
            raise ValueError(f"gain must be a scalar, [P] or [{R}, P]")
        return torch.view_as_real(t.to(torch.complex64).contiguous())
    a = _path_array(v, R, "gain").astype(np.complex64)
    return torch.from_numpy(np.stack([a.real, a.imag], axis=-1).astype(np.float32)).to(dev)


def _row_words64(v, R: int, dev: torch.device, name: str, conv) -> Optional[torch.Tensor]:
    """A per-row 64-bit word parameter: None, or a contiguous [R] int64 tensor on ``dev``.  A
    Python int or an int64 tensor is taken as words; a host float goes through ``conv``."""
    if v is None:
        return None
    if isinstance(v, torch.Tensor):
        if v.dim() > 1 or (v.dim() == 1 and v.shape[0] not in (1, R)):
            raise ValueError(f"{name} must be a scalar or one value per row ([{R}])")
        if v.device != dev:
            raise ValueError(f"{name} is on {v.device}, the samples are on {dev}")
        if v.dtype != torch.int64:
            raise TypeError(f"a {name} tensor holds int64 words; give cycles as host values")
        return (v.reshape(-1).expand(R) if v.numel() == 1 else v).contiguous()
    a = np.asarray(v, dtype=object).reshape(-1)
    if a.size not in (1, R):
        raise ValueError(f"{name} must be a scalar or one value per row ([{R}])")
    w = [int(x) if isinstance(x, (int, np.integer)) and not isinstance(x, bool) else conv(x) for x in a.tolist()]
    if any(not -(1 << 63) <= x < 1 << 63 for x in w):
        raise ValueError(f"a {name} word must fit int64")
    return torch.from_numpy(np.broadcast_to(np.array(w, np.int64), (R,)).copy()).to(dev)


def propagate(iq: torch.Tensor, *, delay=0.0, gain=1.0, sfo_ppm=None, cfo=None, drift=None, phase=None, table=None,
              in_first: int = 0, first_sample: int = 0, length: Optional[int] = None,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Propagation between a transmitter and a receiver, one kernel (lora_propagate_batch; the
    exact arithmetic is in include/lora_mi355x.h and is this project's own): every output sample
    is the sum of ``P`` paths, each the recording read ``delay`` samples earlier through a
    fractional-delay interpolator and weighted by a complex ``gain``; the reading position slides
    by ``sfo_ppm`` parts per million of a sample per sample (a transmitter whose sample clock is
    slow by that much: a frame planted at sample ``s`` arrives near ``s + delay + sfo * s``); and
    the sum is rotated by a carrier offset ``cfo`` (cycles per sample) that drifts by ``drift``
    (cycles per sample, per sample: ``hz_per_s / fs**2``) from a starting ``phase`` (cycles), a
    64-bit phase accumulator that is continuous across chunks by construction.

    ``iq``: [L] or [R, L] complex64 CUDA samples (unit sample stride, rows that do not overlap),
    element ``j`` being sample ``in_first + j`` of the clean recording; whatever lies outside
    reads as zero.  The result is [length] or [R, length] (default ``L``), element ``t`` being
    sample ``first_sample + t`` of the received recording: a recording propagated in chunks, each
    from a window of ``iq`` that covers its paths' taps, is bit for bit the recording propagated
    at once.  ``out``: a complex64 tensor of the result's shape to write into; it must not share
    memory with ``iq``.

    ``delay`` and ``gain``: a scalar, one value per path ([P]) or per row and path ([R, P]); the
    two broadcast against each other.  Host delays are in samples (``delay_word``; negative is an
    advance); an int64 tensor on the device is taken as words, a float tensor is rounded there,
    and a tensor's range (``|delay| <= 2**15`` samples) is the caller's contract, since nothing
    is read back.  ``sfo_ppm``: a scalar or one value per row, host values in parts per million
    (``sfo_word``); a tensor on the device as a delay tensor is - int64 holds words of 2**-32 sample
    per sample, a float tensor parts per million rounded there, its range (``|sfo| <= 2**20``
    words) the caller's contract.  ``cfo`` and
    ``drift``: a scalar or one per row, floats through ``cfo_word64`` (``drift`` is the same unit
    per sample; ``drift_word`` converts Hz per second), Python ints and int64 tensors as words.
    ``phase``: as ``impair``'s.  The rotation with ``drift=None`` is ``impair``'s bit for bit when
    ``cfo`` is a multiple of 2**-32.  ``table``: [256, taps] float32, numpy or on the device
    (default ``fracdelay_table()``, kept per device).

    One kernel on the current stream; it never synchronises and never reads device memory on the
    host.  The channel of a simulated link is ``transmit_wideband`` (or ``modulate_preamble``) ->
    ``propagate`` -> ``impair`` (noise, and the quantiser when ``dtype`` is given) ->
    ``receive_*``; ``propagate``'s ``cfo`` and ``impair``'s add.

    Not covered: time-varying path gains, and DC offset, IQ imbalance or any other front-end
    effect."""
    _require_cuda(iq, "iq")
    one = iq.dim() == 1
    dev = iq.device
    x = _check_iq(iq, dev)
    R, L = x.shape
    W = L if length is None else int(length)
    in_first, first_sample = int(in_first), int(first_sample)
    if W < 0 or in_first < 0 or first_sample < 0:
        raise ValueError("length, in_first and first_sample must be >= 0")
    if W >= 1 << 31 or first_sample + W > 1 << 40 or in_first > 1 << 41:
        raise ValueError("length must be < 2**31, first_sample + length <= 2**40 and in_first <= 2**41")
    d_t, g_t = _path_delay(delay, R, dev), _path_gain(gain, R, dev)
    P = max(d_t.shape[1], g_t.shape[1])
    if d_t.shape[1] not in (1, P) or g_t.shape[1] not in (1, P) or not 1 <= P <= 8:
        raise ValueError("delay and gain must agree on the number of paths, 1..8")
    d_t = d_t.expand(R, P).contiguous()
    g_t = g_t.expand(R, P, 2).contiguous()
    if sfo_ppm is None:
        s_t = None
    elif isinstance(sfo_ppm, torch.Tensor):
        # as a delay tensor: int64 holds words, a float tensor parts per million, rounded on the device
        if sfo_ppm.dtype != torch.int64:
            if not sfo_ppm.is_floating_point():
                raise TypeError("an sfo_ppm tensor is int64 (words of 2**-32 sample per sample) or floating (ppm)")
            sfo_ppm = torch.round(sfo_ppm.to(torch.float64) * (1e-6 * 4294967296.0)).to(torch.int64)
        s_t = _row_words64(sfo_ppm, R, dev, "sfo_ppm", sfo_word)
    else:
        a = np.asarray(sfo_ppm, np.float64).reshape(-1)
        if a.size not in (1, R):
            raise ValueError(f"sfo_ppm must be a scalar or one value per row ([{R}])")
        s_t = torch.from_numpy(np.broadcast_to(np.array([sfo_word(v) for v in a.tolist()], np.int64), (R,)).copy())
        s_t = s_t.to(dev)
    f_t = _row_words64(cfo, R, dev, "cfo", cfo_word64)
    r_t = _row_words64(drift, R, dev, "drift", cfo_word64)
    p_t = _row_values(phase, R, dev, "phase", True)
    if table is None:
        key = (dev.type, dev.index)
        if key not in _default_tables:
            _default_tables[key] = torch.from_numpy(fracdelay_table()).to(dev)
        tab = _default_tables[key]
    elif isinstance(table, torch.Tensor):
        if table.device != dev or table.dtype != torch.float32 or table.dim() != 2 or not table.is_contiguous():
            raise ValueError(f"table must be a contiguous float32 [256, taps] tensor on {dev}")
        tab = table
    else:
        tab = torch.from_numpy(np.ascontiguousarray(table, np.float32)).to(dev)
    if tab.dim() != 2 or tab.shape[0] != 256 or tab.shape[1] < 2 or tab.shape[1] > 32 or tab.shape[1] % 2:
        raise ValueError("table must be [256, taps] with taps even and in 2..32")
    lead = () if one else (R,)
    if out is None:
        out = torch.empty(lead + (W,), dtype=torch.complex64, device=dev)
    else:
        _require_cuda(out, "out")
        if out.dtype != torch.complex64:
            raise TypeError("out must be complex64")
        ok = out.device == dev and tuple(out.shape) == lead + (W,)
        if ok and W > 1:
            ok = out.stride(len(lead)) == 1
        if ok and R > 1 and not one:
            ok = out.stride(0) >= W
        if not ok:
            raise ValueError(f"out must be a complex64 {list(lead + (W,))} tensor on {dev} with unit stride within "
                             "a row and rows that do not overlap")
    if R == 0 or W == 0:
        return out  # nothing to launch (and an empty tensor has no address to pass)
    in_stride = x.stride(0) if R > 1 else L
    out_stride = out.stride(0) if (not one and R > 1) else W
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    got = _capi.lib().lora_propagate_batch(x.data_ptr() if L else None, R, L, in_stride, in_first, W, first_sample, P,
                                           d_t.data_ptr(), g_t.data_ptr(), ptr(s_t), tab.data_ptr(), tab.shape[1],
                                           ptr(f_t), ptr(r_t), ptr(p_t), out.data_ptr(), out_stride, dev.index,
                                           _stream_handle(dev))
    got = _capi.check(got)
    assert got == W, (got, W)
    return out
