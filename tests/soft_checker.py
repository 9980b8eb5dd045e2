"""Host checker of the soft-decision receive path (tests only).

A numpy restatement of the two definitions in include/lora_mi355x.h:

* ``soft_bits`` - lora_demod_soft_bits_batch for one spectrum: per bit c of
  grayToBinary16(k), the two maxima of Q[k] = |X[k]|^2 (> 0, else 0) and one fp32 subtraction.
  ``soft_bits_frames`` applies it to ``Oracle().fft`` of the windows
  ``detect_checker.frame_windows`` builds, so everything below the maxima is what
  tests/detect_checker.py and the oracle's fft already pin to the reference.
* ``decode_chain_soft`` - lora_decode_chain_soft_batch: the chain's deinterleave map and
  whitening sequence (lora_phy_amd/codes.py) applied to LLRs, then the nibble whose codeword
  has the largest metric; the metric's fp32 additions run one bit at a time, in bit order.

Every fp32 operation is a separate numpy float32 operation.  Comparisons against the GPU are
on bit patterns (detect_checker.bits).
"""
from __future__ import annotations

import numpy as np

from lora_phy_amd import codes
from tests import detect_checker as dc

F32 = np.float32


def spectrum_q(X: np.ndarray) -> np.ndarray:
    """Q[k] = P[k] > 0 ? P[k] : 0 with P = re*re + im*im in fp32 (LoRaDetector.hpp:51-57)."""
    re, im = X.real.astype(F32), X.imag.astype(F32)
    with np.errstate(all="ignore"):
        p = re * re + im * im
        return np.where(p > 0, p, F32(0)).astype(F32)


def hard_index(X: np.ndarray) -> int:
    """The detector's index: the first maximum of Q (detect_checker.detect's, without its tail)."""
    return int(np.argmax(spectrum_q(X)))


def soft_bits(X: np.ndarray, sf: int) -> np.ndarray:
    """[sf] float32 LLRs of one N = 2^sf point spectrum."""
    q = spectrum_q(X)
    v = codes.gray_to_binary16(np.arange(len(q), dtype=np.uint16)).astype(np.int64)
    out = np.zeros(sf, F32)
    with np.errstate(all="ignore"):
        for c in range(sf):
            one = ((v >> c) & 1) == 1
            m1, m0 = F32(q[one].max()), F32(q[~one].max())
            out[c] = F32(0) if m1 == m0 else F32(m1 - m0)
    return out


def soft_bits_frames(M, x2d: np.ndarray, sf: int, osr: int = 1, mode: str = "legacy", hann: bool = False,
                     dechirp: bool = False, bw: int = 125000, cfo=None, time_offset=None, max_amp=None,
                     with_index: bool = False):
    """[F, total, sf] float32 for a [F, L] batch (and the [F, total] hard indices on request)."""
    x2d = np.ascontiguousarray(x2d, np.complex64)
    F, L = x2d.shape
    total = L // ((1 << sf) * osr)
    llr = np.zeros((F, total, sf), F32)
    idx = np.zeros((F, total), np.uint16)
    for f in range(F):
        w = dc.frame_windows(M, x2d[f], sf, osr, mode, hann, dechirp, bw,
                             0.0 if cfo is None else cfo[f], 0.0 if time_offset is None else time_offset[f],
                             0.0 if max_amp is None else max_amp[f])
        for s in range(total):
            X = M.fft(w[s])
            llr[f, s] = soft_bits(X, sf)
            idx[f, s] = hard_index(X)
    return (llr, idx) if with_index else llr


def chain_llrs(llr: np.ndarray, sf: int, rdd: int) -> np.ndarray:
    """[S, sf] symbol LLRs -> [blocks * sf, 4 + rdd] codeword LLRs: diagonalDeterleaveSx's map
    (codes.diagonal_deinterleave) and the chain's whitening as sign flips."""
    llr = np.asarray(llr, F32)
    nb = 4 + rdd
    nblk = llr.shape[0] // nb
    L = np.zeros((nblk * sf, nb), F32)
    blk, bit, c = np.meshgrid(np.arange(nblk), np.arange(nb), np.arange(sf), indexing="ij")
    L[blk * sf + (c + bit) % sf, bit] = llr[blk * nb + bit, c]
    w = np.frombuffer(codes.sx1272_whitening_lfsr(bytes(nblk * sf), 0, rdd), np.uint8)
    flip = ((w[:, None] >> np.arange(nb)[None, :]) & 1) == 1
    return np.where(flip, -L, L).astype(F32)


def decode_chain_soft(llr: np.ndarray, sf: int, rdd: int, nbytes: int):
    """(payload uint8 [nbytes], corrected) of one frame's [S, sf] LLRs."""
    nb = 4 + rdd
    L = chain_llrs(llr, sf, rdd)[: 2 * nbytes]
    assert len(L) == 2 * nbytes, "nbytes needs more codewords than the symbols yield"
    cw = codes.nibble_encode(np.arange(16), rdd).astype(np.int64)         # [16]
    ebit = ((cw[:, None] >> np.arange(nb)[None, :]) & 1) == 1            # [16, nb]
    with np.errstate(all="ignore"):
        m = np.zeros((len(L), 16), F32)                                   # +0.0f
        for b in range(nb):                                               # in bit order
            m = (m + np.where(ebit[None, :, b], L[:, b, None], -L[:, b, None]).astype(F32)).astype(F32)
        best = np.full(len(L), -np.inf, F32)
        nib = np.zeros(len(L), np.int64)
        for x in range(16):                                               # strict '>', upward
            up = m[:, x] > best
            best = np.where(up, m[:, x], best)
            nib = np.where(up, x, nib)
        hard = ((L > 0).astype(np.int64) << np.arange(nb)[None, :]).sum(axis=1)
    corrected = int((cw[nib] != hard).sum())
    pay = ((nib[0::2] << 4) | nib[1::2]).astype(np.uint8)
    return pay, corrected


def decode_chain_soft_frames(llr3: np.ndarray, sf: int, rdd: int, nbytes: int):
    """([F, nbytes] uint8, [F] int32) of a [F, S, sf] batch."""
    res = [decode_chain_soft(row, sf, rdd, nbytes) for row in llr3]
    return (np.stack([p for p, _ in res]).reshape(len(res), nbytes), np.array([c for _, c in res], np.int32))


# ---- frames for the tests --------------------------------------------------------------------
def noise_sigma(snr_db: float) -> float:
    """Per-component noise sigma of the soft path's tests and tools for a unit-amplitude
    signal: 10^(-snr/20) on I and on Q each.  (awgn.sweep_chain divides the same figure by
    sqrt(2): a point labelled s dB here carries the noise of its s - 3.01 dB point.)"""
    return 10.0 ** (-snr_db / 20.0)


def chain_frames(M, sf: int, rdd: int, payloads: np.ndarray, snr_db=None, rng=None):
    """Modulated frames of the chain's symbols for [F, n] payload bytes, with complex white
    noise of ``noise_sigma(snr_db)`` per component when ``snr_db`` is given."""
    rows = []
    for p in payloads:
        syms = codes.encode_chain(p.tobytes(), sf, rdd)["symbols"]
        rows.append(M.lora_modulate(np.asarray(syms, np.uint16), sf, 1, 125000, 1.0, 0x12))
    x = np.stack(rows).astype(np.complex64)
    if snr_db is not None:
        sigma = noise_sigma(snr_db)
        x = (x + sigma * (rng.standard_normal(x.shape) + 1j * rng.standard_normal(x.shape))).astype(np.complex64)
    return x
