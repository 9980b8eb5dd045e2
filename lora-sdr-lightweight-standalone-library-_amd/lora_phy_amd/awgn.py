"""AWGN sweeps with the demodulation on the GPU (BASELINE.json configs[3]).

Two harnesses, both host-driven with one batched GPU call per SNR point:

``simulate(sf, cr, snr_db, packets, payload_len, up, down)``
    Drop-in for the reference's ``tests/awgn_sweep.py:simulate`` (same signature, same
    ``np.random`` draw order: per packet ``randint(0, 256, L)`` then per symbol
    ``normal(N)`` for I and ``normal(N)`` for Q, awgn_sweep.py:251-267).  The channel
    and the dechirp ``r * down`` are computed in float64 exactly as the script does;
    the per-symbol FFT + argmax runs on the GPU in LORA_MODE_RAW (fp32 kissfft order)
    instead of numpy's float64 FFT.  FEC (CR 4/5 parity, 4/8 Hamming) and the bit <->
    symbol packing restate the script's host code.  Decisions can differ from the
    script's only where two bins' magnitudes tie to within fp32 rounding.

``sweep_chain(sf, snr_dbs, frames, payload_len, seed, cfo_bins=0.0)``
    The library's own chain: ``lora_encode`` (Hamming 8/4 per nibble) -> GPU
    ``lora_modulate`` (2 sync up-chirps + payload) -> complex AWGN with
    sigma = 10^(-SNR/20) (awgn_sweep_gtest.cpp:76-80) and an optional CFO phase ramp
    ``2*pi*cfo_bins*(n mod N)/N`` (lora_phy_vector_generate.cpp:102-108) -> GPU LEGACY
    ``lora_demodulate`` with the caller-side dechirp, i.e. normalisation + the 2-sync-
    symbol CFO/timing estimate + per-symbol CFO rotation (the reference's "preamble
    detect + CFO correct", LoRaDemod.cpp:79-157) -> ``lora_decode``.  Reports SER, BER,
    PER and returns the noisy IQ so callers can check the GPU against the oracle.

``sweep_receive(sf, snr_dbs, frames, frame_symbols, ...)``
    Detection probability of the stream receiver, everything on the device: GPU-modulated
    frames planted at known starts in zero rows -> ``stream.impair`` in place of a copy (counter-
    based AWGN and an optional carrier offset, reproducible on the CPU) -> ``stream.receive_device``
    -> counts of the planted starts returned exactly, of the returned starts that were not
    planted and of the detected frames whose symbols all equal the planted ones.  Noise-only
    batches give false starts per window.  One synchronisation, at the end, for the counts.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import codes
from .demod import DemodPlan
from .mod import modulate

# --------------------------------------------------------------------------------------
# tests/awgn_sweep.py host pieces (restated; pinned by tests/golden/awgn_sweep.json)
# --------------------------------------------------------------------------------------

_WIDTH = {"4/5": 5, "4/8": 8}


def encode_payload(payload: bytes, cr: str) -> np.ndarray:
    """Bits (uint8, LSB-first per codeword) of the high/low nibbles of every byte,
    CR 4/5 = parity54, CR 4/8 = Hamming 8/4 (awgn_sweep.py:139-158)."""
    if cr not in _WIDTH:
        raise ValueError(f"Unsupported coding rate: {cr}")
    b = np.frombuffer(bytes(payload), np.uint8).astype(np.int64)
    nib = np.stack([b >> 4, b & 0xF], 1).reshape(-1)
    cw = (codes.ENC_P54 if cr == "4/5" else codes.ENC_H84)[nib].astype(np.int64)
    w = _WIDTH[cr]
    return ((cw[:, None] >> np.arange(w)) & 1).astype(np.uint8).reshape(-1)


def decode_payload(bits: np.ndarray, cr: str, num_bytes: int) -> np.ndarray:
    """Inverse of encode_payload (CR 4/5: data nibble as received; CR 4/8: Hamming 8/4
    correction of single-bit errors), awgn_sweep.py:161-189."""
    w = _WIDTH[cr]
    b = np.asarray(bits, np.int64)[: num_bytes * 2 * w].reshape(num_bytes * 2, w)
    cw = (b << np.arange(w)).sum(1)
    nib = (cw & 0xF) if cr == "4/5" else codes.decode_hamming84(cw)[0].astype(np.int64)
    return ((nib[0::2] << 4) | nib[1::2]).astype(np.uint8)


def bits_to_symbols(bits: np.ndarray, sf: int) -> np.ndarray:
    """Pack bits LSB-first into sf-bit symbols, zero padded (awgn_sweep.py:197-207)."""
    b = np.asarray(bits, np.int64)
    pad = (-len(b)) % sf
    b = np.concatenate([b, np.zeros(pad, np.int64)]).reshape(-1, sf)
    return (b << np.arange(sf)).sum(1)


def symbols_to_bits(symbols, sf: int, bit_len: int) -> np.ndarray:
    """awgn_sweep.py:210-217."""
    s = np.asarray(symbols, np.int64)
    return ((s[:, None] >> np.arange(sf)) & 1).reshape(-1)[:bit_len].astype(np.uint8)


def make_chirps(sf: int):
    """awgn_sweep.py:225-234: float64 up/down chirps of the Python model."""
    N = 1 << sf
    n = np.arange(N, dtype=float)
    accum = np.cumsum(-math.pi + (2 * math.pi * n) / N)
    up = np.exp(1j * accum)
    return up, np.conj(up)


def simulate(sf: int, cr: str, snr_db: float, packets: int, payload_len: int, up: np.ndarray,
             down: np.ndarray, device=None, return_symbols: bool = False):
    """GPU-demodulated twin of awgn_sweep.py:simulate -> (ber, per)."""
    N = len(up)
    n = np.arange(N)
    sigma = 10 ** (-snr_db / 20.0)
    rows, meta = [], []
    for _ in range(packets):
        payload = np.random.randint(0, 256, payload_len, dtype=np.uint8)
        tx_bits = encode_payload(payload.tobytes(), cr)
        syms = bits_to_symbols(tx_bits, sf)
        for sym in syms:
            shift = np.exp(1j * 2 * math.pi * int(sym) * n / N)
            tx = up * shift
            noise = np.random.normal(size=N) + 1j * np.random.normal(size=N)
            noise *= sigma / math.sqrt(2.0)
            rows.append((tx + noise) * down)
        meta.append((payload, tx_bits, len(syms)))
    iq = torch.from_numpy(np.asarray(rows).astype(np.complex64))
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    plan = DemodPlan(sf, 1, 125000, "none", dechirp=False, mode="raw", device=dev)
    rx = plan.run(iq.to(dev)).symbols[:, 0].to(torch.int64).cpu().numpy()
    bit_errors = packet_errors = total_bits = 0
    off = 0
    for payload, tx_bits, ns in meta:
        rx_bits = symbols_to_bits(rx[off:off + ns], sf, len(tx_bits))
        off += ns
        rx_payload = decode_payload(rx_bits, cr, payload_len)
        diff = np.bitwise_xor(payload, rx_payload)
        bit_errors += int(np.unpackbits(diff).sum())
        total_bits += payload_len * 8
        packet_errors += int(diff.any())
    ber = bit_errors / total_bits if total_bits else 0.0
    per = packet_errors / packets if packets else 0.0
    if return_symbols:
        return ber, per, rx, np.asarray(rows)
    return ber, per


# --------------------------------------------------------------------------------------
# The library chain under AWGN (+ optional CFO)
# --------------------------------------------------------------------------------------

def sweep_chain(sf: int, snr_dbs: Sequence[float], frames: int = 1000, payload_len: int = 16,
                seed: int = 1234, cfo_bins: float = 0.0, osr: int = 1, device=None,
                keep_iq: bool = False, exact_check: bool = False) -> List[Dict]:
    """SER / BER / PER of encode -> modulate -> AWGN (+CFO) -> LEGACY demod -> decode.

    exact_check: also run every point through the three-launch exact path (the oracle-pinned
    kernels, LORA_MI355X_SPEC=0) and count the frames whose symbols, sync word or cfo /
    time_offset bits differ from the default (speculative, certified) pipeline's."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    N = 1 << sf
    rng = np.random.default_rng(seed)
    payloads = rng.integers(0, 256, (frames, payload_len)).astype(np.uint8)
    tx = np.stack([codes.lora_encode(p.tobytes()) for p in payloads]).astype(np.int32)
    clean = modulate(torch.from_numpy(tx).to(dev), sf, osr)
    L = clean.shape[1]
    if cfo_bins:
        nn = torch.arange(L, device=dev, dtype=torch.float64) % (N * osr)
        ph = 2.0 * math.pi * cfo_bins * nn / (N * osr)
        clean = (clean.to(torch.complex128) * torch.polar(torch.ones_like(ph), ph)).to(torch.complex64)
    plan = DemodPlan(sf, osr, 125000, "none", dechirp=True, mode="legacy", device=dev)
    xplan = None
    if exact_check:
        from .demod import spec_pipeline

        with spec_pipeline(False):
            xplan = DemodPlan(sf, osr, 125000, "none", dechirp=True, mode="legacy", device=dev)
    gen = torch.Generator(device=dev).manual_seed(seed + 1)
    out = []
    for snr in snr_dbs:
        sigma = 10.0 ** (-snr / 20.0) / math.sqrt(2.0)
        noise = torch.randn((frames, L, 2), generator=gen, device=dev) * sigma
        iq = clean + torch.view_as_complex(noise)
        fixed0 = plan.spec_recomputed()
        res = plan.run(iq)
        rx = res.symbols.to(torch.int64).cpu().numpy()
        dec = codes.lora_decode(rx)
        # the modulator sends each 8-bit Hamming codeword modulo N (SF7 drops bit 7,
        # which the decoder then corrects), so symbol errors count against tx mod N
        ser = float((rx != (tx % N)).mean())
        diff = np.bitwise_xor(dec, payloads)
        rec = {"sf": sf, "snr_db": float(snr), "frames": frames, "ser": ser,
               "ber": float(np.unpackbits(diff).mean()), "per": float(diff.any(1).mean()),
               "sync_ok": float((res.sync == 0x12).float().mean()), "cfo_bins": cfo_bins,
               "recomputed_symbols": int(plan.spec_recomputed() - fixed0)}
        if xplan is not None:
            rx_ = xplan.run(iq)
            bad = ((res.symbols != rx_.symbols).any(1) | (res.sync != rx_.sync)
                   | (res.cfo.view(torch.int32) != rx_.cfo.view(torch.int32))
                   | (res.time_offset.view(torch.int32) != rx_.time_offset.view(torch.int32)))
            rec["exact_path_frames_compared"] = frames
            rec["exact_path_frame_mismatches"] = int(bad.sum())
        if keep_iq:
            rec["iq"] = iq
            rec["result"] = res
        out.append(rec)
    return out


# --------------------------------------------------------------------------------------
# The stream receiver's detection probability (stream.impair -> stream.receive_device)
# --------------------------------------------------------------------------------------

def sweep_receive(sf: int, snr_dbs: Sequence[float], frames: int = 2000, frame_symbols: int = 16, osr: int = 1,
                  hop: Optional[int] = None, thresh_db: float = 0.0, cfo_bins: float = 0.0, seed: int = 1234,
                  frames_per_row: int = 4, noise_windows: int = 0, noise_batch_samples: int = 1 << 27,
                  sync: int = 0x12, device=None) -> List[Dict]:
    """Detection probability and false starts of ``stream.receive_device`` under ``stream.impair``.

    Layout: ``ceil(frames / frames_per_row)`` zero rows, each with ``frames_per_row`` frames of
    ``frame_symbols`` random data symbols (GPU ``modulate``, amplitude 1) at starts that are
    multiples of ``osr``, every frame after a gap drawn uniformly from 0 .. 2 * step - 1 chips (and
    one such gap behind the last).  The layout and the symbols are drawn once from ``seed`` and
    serve every SNR point; the noise of point i is ``impair``'s with this ``seed`` and ``first_row
    = i * rows``, so no two points share a noise sample.  ``cfo_bins`` is the carrier offset in
    FFT bins (``cfo_bins / (N * osr)`` cycles per sample).  ``hop`` defaults to ``step // 4``.

    Per SNR point one record: ``planted``, ``detected`` (planted starts returned exactly),
    ``false_starts`` (returned starts that were not planted), ``all_symbols_correct`` (detected
    frames whose ``frame_symbols`` symbols all equal the planted ones), ``windows`` (scanned) and
    the rates ``p_detect``, ``p_all_correct_given_detected``.  With ``noise_windows > 0`` a last
    record (``"noise_only": True``) has the false starts over at least that many windows of noise
    alone (``impair(None, ...)`` in batches of about ``noise_batch_samples``).  Everything runs on
    the device; the counts of all points come to the host in one copy at the end."""
    from . import stream

    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    N = 1 << sf
    step = N * osr
    hop = step // 4 if hop is None else int(hop)
    S, K = int(frame_symbols), int(frames_per_row)
    frame_len = (S + 2) * step
    R = -(-int(frames) // K)
    F = R * K
    rng = np.random.default_rng(seed)
    gaps = rng.integers(0, 2 * N, (R, K + 1)) * osr
    starts = np.cumsum(gaps[:, :K], axis=1) + np.arange(K) * frame_len          # [R, K]
    L = int((starts[:, -1] + frame_len + gaps[:, K]).max())
    syms = rng.integers(0, N, (F, S)).astype(np.int32)
    plan = DemodPlan(sf, osr, 125000, "none", dechirp=True, mode="legacy", device=dev)
    starts_t = torch.from_numpy(starts).to(dev)
    syms_t = torch.from_numpy(syms).to(dev).view(R, K, S)
    clean = torch.zeros((R, L), dtype=torch.complex64, device=dev)
    at = (torch.arange(R, device=dev)[:, None] * L + starts_t).reshape(-1)
    clean.view(-1)[at[:, None] + torch.arange(frame_len, device=dev)] = modulate(
        torch.from_numpy(syms).to(dev), sf, osr, 125000, 1.0, sync)
    work = torch.empty_like(clean)
    W = (L - step) // hop + 1
    cfo = float(cfo_bins) / step
    counts = []
    for i, snr in enumerate(snr_dbs):
        stream.impair(clean, snr_db=float(snr), cfo=cfo if cfo_bins else None, seed=seed, first_row=i * R, out=work)
        got = stream.receive_device(plan, work, S, hop, sync, thresh_db)
        valid = got.found.valid                                                  # [R, cap]
        same = got.found.starts[:, :, None] == starts_t[:, None, :]              # [R, cap, K]
        hit = same.any(2) & valid
        which = same.to(torch.int8).argmax(2)                                    # the planted frame of a hit
        want = torch.gather(syms_t, 1, which[:, :, None].expand(-1, -1, S))
        rx = got.result.symbols.to(torch.int32).view(R, -1, S) % N
        right = hit & (rx == want).all(2)
        counts.append(torch.stack([hit.sum(), (valid & ~hit).sum(), right.sum(),
                                   (got.found.count.to(torch.int64) - valid.sum(1)).sum()]))
    noise_counts, noise_total = [], 0
    if noise_windows > 0:
        Ln = max(frame_len + step, min(int(noise_batch_samples), 1 << 24))
        Rn = max(1, int(noise_batch_samples) // Ln)
        Wn = (Ln - step) // hop + 1
        buf = torch.empty((Rn, Ln), dtype=torch.complex64, device=dev)
        b = 0
        while noise_total < noise_windows:
            stream.impair(None, sigma=1.0, seed=seed + 1, first_row=b * Rn, out=buf, rows=Rn, length=Ln, device=dev)
            noise_counts.append(stream.receive_device(plan, buf, S, hop, sync, thresh_db).found.count.sum())
            noise_total += Rn * Wn
            b += 1
    got = torch.stack(counts).cpu().numpy() if counts else np.zeros((0, 4), np.int64)  # the synchronisation
    out = []
    for snr, (hit, false, right, dropped) in zip(snr_dbs, got.tolist()):
        out.append({"sf": sf, "osr": osr, "snr_db": float(snr), "cfo_bins": float(cfo_bins), "hop": hop,
                    "thresh_db": float(thresh_db), "frame_symbols": S, "planted": F, "detected": hit,
                    "false_starts": false, "all_symbols_correct": right, "not_stored": dropped,
                    "windows": R * W, "p_detect": hit / F,
                    "p_all_correct_given_detected": (right / hit) if hit else None})
    if noise_counts:
        false = int(torch.stack(noise_counts).sum().cpu())
        out.append({"sf": sf, "osr": osr, "noise_only": True, "hop": hop, "thresh_db": float(thresh_db),
                    "frame_symbols": S, "windows": noise_total, "false_starts": false,
                    "false_starts_per_million_windows": false * 1e6 / noise_total})
    return out


# --------------------------------------------------------------------------------------
# Self-describing frames of mixed lengths (stream.impair -> stream.receive_frames_device)
# --------------------------------------------------------------------------------------

def sweep_receive_frames(sf: int, snr_dbs: Sequence[float], frames: int = 1000, max_bytes: int = 16, cr=1,
                         osr: int = 1, hop: Optional[int] = None, thresh_db: float = 0.0, seed: int = 1234,
                         frames_per_row: int = 4, noise_windows: int = 0, noise_batch_samples: int = 1 << 26,
                         sync: int = 0x12, device=None, soft: bool = False, max_flips: int = 5,
                         cfo_bins: float = 0.0) -> List[Dict]:
    """``sweep_receive`` for frames that state their own length: what ``stream.receive_frames_device``
    returns under ``stream.impair``, with no frame length given to it.

    Layout: ``ceil(frames / frames_per_row)`` zero rows, each with ``frames_per_row`` self-describing
    frames (``codec.encode_frame`` at coding rate ``cr`` with the CRC, GPU ``modulate``, amplitude
    1) whose payload lengths are drawn uniformly from 0 .. ``max_bytes`` - mixed lengths in every
    row - at starts that are multiples of ``osr``, every frame after a gap drawn uniformly from
    0 .. 2 * step - 1 chips (and one such gap behind the last).  The layout and the payloads are
    drawn once from ``seed`` and serve every SNR point; the noise of point i is ``impair``'s with
    this ``seed`` and ``first_row = i * rows``.  ``max_symbols`` is that of a ``max_bytes`` frame.

    Per SNR point one record: ``planted``; ``returned_ok`` - planted frames returned at their exact
    start with status OK and the exact payload (``p_ok``); ``found_at_planted`` - planted starts
    among the returned, whatever their decode; ``false_frames`` - returned frames whose start was
    not planted (``false_frames_per_million_windows``), ``false_frames_ok`` those of them whose
    status is OK; ``candidates`` listed and ``candidates_dropped`` beyond the candidate capacity;
    ``windows`` scanned.  With ``noise_windows > 0`` a last record (``"noise_only": True``) has the
    candidates and the false frames over at least that many windows of noise alone.  Everything
    runs on the device; the counts of all points come to the host in one copy at the end.

    ``soft`` and ``max_flips`` go to ``receive_frames_device``: the rows and their noise do not
    depend on them, so the same seeded rows can be received both ways.  The records carry them.
    ``cfo_bins``: a carrier offset of that many bins (``cfo_bins / step`` cycles per sample) put on
    the rows by the same ``impair`` call; 0 (the default) performs no rotation at all."""
    from . import codec, stream

    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    N = 1 << sf
    step = N * osr
    hop = step // 4 if hop is None else int(hop)
    K, B = int(frames_per_row), int(max_bytes)
    R = -(-int(frames) // K)
    F = R * K
    S = codec.frame_symbols(sf, cr, B)
    rng = np.random.default_rng(seed)
    nbytes = rng.integers(0, B + 1, (R, K))
    nsym = np.vectorize(lambda n: codec.frame_symbols(sf, cr, int(n)))(nbytes)
    length = (nsym + 2) * step                                                   # [R, K]
    gaps = rng.integers(0, 2 * N, (R, K + 1)) * osr
    starts = np.cumsum(gaps[:, :K], axis=1) + np.cumsum(length, axis=1) - length
    L = int((starts[:, -1] + length[:, -1] + gaps[:, K]).max())
    pay = rng.integers(0, 256, (F, B)).astype(np.uint8)
    pay[np.arange(B)[None, :] >= nbytes.reshape(-1, 1)] = 0
    plan = DemodPlan(sf, osr, 125000, "none", dechirp=True, mode="legacy", device=dev)
    starts_t = torch.from_numpy(starts).to(dev)
    pay_t = torch.from_numpy(pay).to(dev).view(R, K, B)
    nbytes_t = torch.from_numpy(nbytes.astype(np.int32)).to(dev)
    symbols, _ = codec.encode_frame(pay_t.view(F, B), nbytes_t.view(-1), sf, cr)
    rows = modulate(symbols, sf, osr, 125000, 1.0, sync)                         # [F, (S + 2) * step]
    clean = torch.zeros((R, L), dtype=torch.complex64, device=dev)
    at = (torch.arange(R, device=dev)[:, None] * L + starts_t).reshape(-1)
    live = torch.arange(rows.shape[1], device=dev)[None, :] < torch.from_numpy(length).to(dev).reshape(-1, 1)
    clean.view(-1)[(at[:, None] + torch.arange(rows.shape[1], device=dev))[live]] = rows[live]
    del rows, live
    work = torch.empty_like(clean)
    W = (L - step) // hop + 1
    counts = []

    def tally(got):
        valid = got.found.valid                                                  # [R, cap]
        cap = valid.shape[1]
        same = got.found.starts[:, :, None] == starts_t[:, None, :]              # [R, cap, K]
        hit = same.any(2) & valid
        which = same.to(torch.int8).argmax(2)
        ok = got.frames.status.view(R, cap) == codec.FRAME_OK
        want = torch.gather(pay_t, 1, which[:, :, None].expand(-1, -1, B))
        want_n = torch.gather(nbytes_t, 1, which)
        rx = got.frames.payload.view(R, cap, got.frames.payload.shape[-1])[:, :, :B]
        right = hit & ok & (got.frames.nbytes.view(R, cap) == want_n) & (rx == want).all(2)
        C = got.found.starts.new_tensor(-(-L // (4 * step)))
        return torch.stack([right.sum(), hit.sum(), (valid & ~hit).sum(), (valid & ~hit & ok).sum(),
                            got.candidates.sum(), (got.candidates.to(torch.int64) - C).clamp_min(0).sum()])

    for i, snr in enumerate(snr_dbs):
        stream.impair(clean, snr_db=float(snr), seed=seed, first_row=i * R, out=work,
                      cfo=(float(cfo_bins) / step) if cfo_bins else None)
        counts.append(tally(stream.receive_frames_device(plan, work, S, hop, sync, thresh_db, soft=soft,
                                                         max_flips=max_flips)))
    noise_counts, noise_total = [], 0
    if noise_windows > 0:
        Ln = max((S + 3) * step, min(int(noise_batch_samples), 1 << 22))
        Rn = max(1, int(noise_batch_samples) // Ln)
        Wn = (Ln - step) // hop + 1
        Cn = -(-Ln // (4 * step))
        buf = torch.empty((Rn, Ln), dtype=torch.complex64, device=dev)
        b = 0
        while noise_total < noise_windows:
            stream.impair(None, sigma=1.0, seed=seed + 1, first_row=b * Rn, out=buf, rows=Rn, length=Ln, device=dev)
            got = stream.receive_frames_device(plan, buf, S, hop, sync, thresh_db, soft=soft, max_flips=max_flips)
            ok = (got.frames.status.view(Rn, -1) == codec.FRAME_OK) & got.found.valid
            noise_counts.append(torch.stack([got.found.count.sum(), ok.sum(), got.candidates.sum(),
                                             (got.candidates.to(torch.int64) - Cn).clamp_min(0).sum()]))
            noise_total += Rn * Wn
            b += 1
    got = torch.stack(counts).cpu().numpy() if counts else np.zeros((0, 6), np.int64)  # the synchronisation
    out = []
    for snr, (right, hit, false, false_ok, cands, dropped) in zip(snr_dbs, got.tolist()):
        out.append({"sf": sf, "osr": osr, "snr_db": float(snr), "hop": hop, "thresh_db": float(thresh_db),
                    "max_bytes": B, "max_symbols": S, "rdd": codes.rdd_of(cr), "planted": F, "returned_ok": right,
                    "found_at_planted": hit, "false_frames": false, "false_frames_ok": false_ok,
                    "candidates": cands, "candidates_dropped": dropped, "windows": R * W, "p_ok": right / F,
                    "false_frames_per_million_windows": false * 1e6 / (R * W)})
    if noise_counts:
        false, false_ok, cands, dropped = torch.stack(noise_counts).sum(0).cpu().tolist()
        out.append({"sf": sf, "osr": osr, "noise_only": True, "hop": hop, "thresh_db": float(thresh_db),
                    "max_symbols": S, "windows": noise_total, "false_frames": false, "false_frames_ok": false_ok,
                    "candidates": cands, "candidates_dropped": dropped,
                    "candidates_per_window": cands / noise_total,
                    "candidate_capacity_per_window": hop / (4 * step),
                    "false_frames_per_million_windows": false * 1e6 / noise_total})
    if soft:
        for rec in out:
            rec.update(soft=True, max_flips=int(max_flips))
    return out


def sweep_receive_preamble(sf: int, snr_dbs: Sequence[float], frames: int = 1000, max_bytes: int = 16, cr=1,
                           osr: int = 1, hop: Optional[int] = None, thresh_up_db: float = 0.0,
                           thresh_dn_db: float = 0.0, preamble: int = 8, preamble_acc: int = 6,
                           cfo_bins: float = 0.0, max_cfo_bins: Optional[int] = None, seed: int = 1234,
                           frames_per_row: int = 4, noise_windows: int = 0, noise_batch_samples: int = 1 << 26,
                           sync: int = 0x12, device=None, soft: bool = False, max_flips: int = 5,
                           cand_capacity_mult: int = 1, propagate: Optional[Dict] = None) -> List[Dict]:
    """``sweep_receive_frames`` for preambled frames: what ``stream.receive_preamble_frames_device``
    returns under ``stream.impair`` with a carrier offset of ``cfo_bins`` bins.  The payloads, their
    lengths and the gaps are drawn from ``seed`` in ``sweep_receive_frames``' order, so the two
    sweeps carry the same payloads; here every frame has ``preamble`` up-chirps in front and the
    delimiter inside (``modulate_preamble``), and a planted start is the frame's first sync symbol.

    The records are ``sweep_receive_frames``' plus ``cfo_right``: the planted frames returned with
    the exact payload whose reported offset is ``round(cfo_bins)`` (``returned_ok`` does not ask for
    it).  The noise-only record counts the candidates of the preamble finder.
    ``cand_capacity_mult``: the candidate capacity as a multiple of the chain's default (one slot
    per four symbols of the row), to tell frames lost to a full candidate list from frames not
    found; ``candidates_dropped`` counts against the capacity used.

    ``propagate``: a dict of ``stream.propagate`` keyword arguments (host values: ``delay`` a scalar,
    [P] or [R, P], ``sfo_ppm`` and ``cfo`` scalars or one per row), applied once to the clean rows
    before the SNR loop; the records then carry it as ``"propagate"``.  With ``None`` nothing is
    applied and every record is what it was, bit for bit.  A channel moves a frame, so with one a
    planted frame counts as found when a returned start lies within one chip (``osr`` samples) of
    ``planted + delay + sfo * planted`` - ``delay`` the first path's and ``sfo`` the clock offset as
    a fraction - instead of on the planted sample itself, and ``cfo_right`` asks for
    ``round(cfo_bins + cfo * step)``."""
    from . import codec, stream
    from .mod import modulate_preamble

    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    N = 1 << sf
    step = N * osr
    tail = 9 * step // 4
    hop = step // 4 if hop is None else int(hop)
    K, B, P = int(frames_per_row), int(max_bytes), int(preamble)
    R = -(-int(frames) // K)
    F = R * K
    S = codec.frame_symbols(sf, cr, B)
    rng = np.random.default_rng(seed)
    nbytes = rng.integers(0, B + 1, (R, K))
    nsym = np.vectorize(lambda n: codec.frame_symbols(sf, cr, int(n)))(nbytes)
    length = (P + 2 + nsym) * step + tail                                        # [R, K]
    gaps = rng.integers(0, 2 * N, (R, K + 1)) * osr
    begins = np.cumsum(gaps[:, :K], axis=1) + np.cumsum(length, axis=1) - length
    starts = begins + P * step                                                   # the first sync symbol
    L = int((begins[:, -1] + length[:, -1] + gaps[:, K]).max())
    pay = rng.integers(0, 256, (F, B)).astype(np.uint8)
    pay[np.arange(B)[None, :] >= nbytes.reshape(-1, 1)] = 0
    plan = DemodPlan(sf, osr, 125000, "none", dechirp=True, mode="legacy", device=dev)
    starts_t = torch.from_numpy(starts).to(dev)
    pay_t = torch.from_numpy(pay).to(dev).view(R, K, B)
    nbytes_t = torch.from_numpy(nbytes.astype(np.int32)).to(dev)
    symbols, _ = codec.encode_frame(pay_t.view(F, B), nbytes_t.view(-1), sf, cr)
    rows = modulate_preamble(symbols, sf, osr, 125000, 1.0, sync, P)             # [F, (P + 2 + S) * step + tail]
    clean = torch.zeros((R, L), dtype=torch.complex64, device=dev)
    at = (torch.arange(R, device=dev)[:, None] * L + torch.from_numpy(begins).to(dev)).reshape(-1)
    live = torch.arange(rows.shape[1], device=dev)[None, :] < torch.from_numpy(length).to(dev).reshape(-1, 1)
    clean.view(-1)[(at[:, None] + torch.arange(rows.shape[1], device=dev))[live]] = rows[live]
    del rows, live
    want_c = int(round(float(cfo_bins)))
    moved_t = None
    if propagate is not None:
        # the scoring needs the channel's numbers on the host: tensors and shapes it cannot read are refused
        for k in ("delay", "sfo_ppm", "cfo"):
            if isinstance(propagate.get(k), torch.Tensor):
                raise TypeError(f"propagate[{k!r}] must be a host value here: the scoring reads it")
        d0 = np.asarray(propagate.get("delay", 0.0), np.float64)
        d0 = d0.reshape(1, 1) if d0.ndim == 0 else d0.reshape(1, -1) if d0.ndim == 1 else d0
        if d0.ndim != 2 or d0.shape[0] not in (1, R) or d0.shape[1] < 1:
            raise ValueError(f"propagate['delay'] must be a scalar, [P] or [{R}, P]")
        sfo = propagate.get("sfo_ppm")
        sfo = np.asarray(0.0 if sfo is None else sfo, np.float64)
        if sfo.ndim > 1 or (sfo.ndim == 1 and sfo.shape[0] not in (1, R)):
            raise ValueError(f"propagate['sfo_ppm'] must be a scalar or one value per row ([{R}])")
        sfo = sfo.reshape(-1, 1) * 1e-6
        c = propagate.get("cfo")
        if c is not None:
            if isinstance(c, (bool, np.bool_)) or not isinstance(c, (int, float, np.integer, np.floating)):
                raise ValueError("propagate['cfo'] must be one number here (a float in cycles per sample, an int a "
                                 "word): cfo_right asks for one offset")
            cycles = float(c) / 18446744073709551616.0 if isinstance(c, (int, np.integer)) else float(c)
            want_c = int(round(float(cfo_bins) + cycles * step))
        clean = stream.propagate(clean, **propagate)
        L = int(clean.shape[1])
        moved_t = torch.from_numpy(np.broadcast_to(starts + d0[:, :1] + sfo * starts, starts.shape).copy()).to(dev)
    work = torch.empty_like(clean)
    W = (L - step) // hop + 1
    counts = []

    mult = int(cand_capacity_mult)

    def receive(x):
        return stream.receive_preamble_frames_device(plan, x, S, preamble_acc, hop, sync, thresh_up_db, thresh_dn_db,
                                                     max_cfo_bins, cand_capacity=mult * -(-x.shape[1] // (4 * step)),
                                                     soft=soft, max_flips=max_flips)

    def tally(got):
        valid = got.found.valid                                                  # [R, cap]
        cap = valid.shape[1]
        if moved_t is None:
            same = got.found.starts[:, :, None] == starts_t[:, None, :]          # [R, cap, K]
        else:
            same = (got.found.starts[:, :, None].to(torch.float64) - moved_t[:, None, :]).abs() <= osr
        hit = same.any(2) & valid
        which = same.to(torch.int8).argmax(2)
        ok = got.frames.status.view(R, cap) == codec.FRAME_OK
        want = torch.gather(pay_t, 1, which[:, :, None].expand(-1, -1, B))
        want_n = torch.gather(nbytes_t, 1, which)
        rx = got.frames.payload.view(R, cap, got.frames.payload.shape[-1])[:, :, :B]
        right = hit & ok & (got.frames.nbytes.view(R, cap) == want_n) & (rx == want).all(2)
        C = got.found.starts.new_tensor(mult * -(-L // (4 * step)))
        return torch.stack([right.sum(), hit.sum(), (valid & ~hit).sum(), (valid & ~hit & ok).sum(),
                            got.candidates.sum(), (got.candidates.to(torch.int64) - C).clamp_min(0).sum(),
                            (right & (got.cfo_bins == want_c)).sum()])

    for i, snr in enumerate(snr_dbs):
        stream.impair(clean, snr_db=float(snr), seed=seed, first_row=i * R, out=work,
                      cfo=(float(cfo_bins) / step) if cfo_bins else None)
        counts.append(tally(receive(work)))
    noise_counts, noise_total = [], 0
    if noise_windows > 0:
        Ln = max((P + S + 6) * step, min(int(noise_batch_samples), 1 << 22))
        Rn = max(1, int(noise_batch_samples) // Ln)
        Wn = (Ln - step) // hop + 1
        Cn = mult * -(-Ln // (4 * step))
        buf = torch.empty((Rn, Ln), dtype=torch.complex64, device=dev)
        b = 0
        while noise_total < noise_windows:
            stream.impair(None, sigma=1.0, seed=seed + 1, first_row=b * Rn, out=buf, rows=Rn, length=Ln, device=dev)
            got = receive(buf)
            ok = (got.frames.status.view(Rn, -1) == codec.FRAME_OK) & got.found.valid
            noise_counts.append(torch.stack([got.found.count.sum(), ok.sum(), got.candidates.sum(),
                                             (got.candidates.to(torch.int64) - Cn).clamp_min(0).sum()]))
            noise_total += Rn * Wn
            b += 1
    got = torch.stack(counts).cpu().numpy() if counts else np.zeros((0, 7), np.int64)  # the synchronisation
    out = []
    common = {"sf": sf, "osr": osr, "hop": hop, "thresh_up_db": float(thresh_up_db),
              "thresh_dn_db": float(thresh_dn_db), "preamble": P, "preamble_acc": int(preamble_acc),
              "cfo_bins": float(cfo_bins), "max_symbols": S, "cand_capacity_mult": mult}
    if propagate is not None:
        # (as JSON takes it: a complex gain as [re, im])
        plain = lambda a: np.stack([a.real, a.imag], -1).tolist() if a.dtype.kind == "c" else a.tolist()  # noqa: E731
        common["propagate"] = {k: plain(np.asarray(v)) for k, v in propagate.items()}
    for snr, (right, hit, false, false_ok, cands, dropped, cfo_right) in zip(snr_dbs, got.tolist()):
        out.append(dict(common, snr_db=float(snr), max_bytes=B, rdd=codes.rdd_of(cr), planted=F, returned_ok=right,
                        cfo_right=cfo_right, found_at_planted=hit, false_frames=false, false_frames_ok=false_ok,
                        candidates=cands, candidates_dropped=dropped, windows=R * W, p_ok=right / F,
                        false_frames_per_million_windows=false * 1e6 / (R * W)))
    if noise_counts:
        false, false_ok, cands, dropped = torch.stack(noise_counts).sum(0).cpu().tolist()
        out.append(dict(common, noise_only=True, windows=noise_total, false_frames=false, false_frames_ok=false_ok,
                        candidates=cands, candidates_dropped=dropped, candidates_per_window=cands / noise_total,
                        candidate_capacity_per_window=hop / (4 * step),
                        false_frames_per_million_windows=false * 1e6 / noise_total))
    if soft:
        for rec in out:
            rec.update(soft=True, max_flips=int(max_flips))
    return out
