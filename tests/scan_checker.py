"""Host model of the stream receive path (tests only).

``scan_host``: the sliding detector scan as the existing checker computes it - every window of
``step`` samples, one every ``hop``, stacked as one-symbol frames and given to
``detect_checker.frames_metrics`` in "raw" mode (LoRaDetector.hpp:39-74 on the oracle's FFT).
``find_frames_host``: the finder's rule (lora_phy_amd/stream.py's docstring) restated in
numpy, window by window.  ``planted_stream``: oracle-modulated frames written into zeros.
"""
from __future__ import annotations

import numpy as np

from tests import detect_checker as dc

FIELDS = ("index", "power", "power_avg", "f_index")


def scan_windows(row_len: int, step: int, hop: int) -> int:
    return 0 if row_len < step else (row_len - step) // hop + 1


def scan_host(O, x, sf: int, osr: int = 1, hop: int = 1, hann: bool = False, dechirp: bool = False,
              bw: int = 125000):
    """dict of [rows, W] arrays (index uint16; power, power_avg, f_index float32) for a [L] or
    [rows, L] stream."""
    x = np.ascontiguousarray(x, np.complex64)
    if x.ndim == 1:
        x = x[None]
    rows, L = x.shape
    step = (1 << sf) * osr
    W = scan_windows(L, step, hop)
    if W == 0:
        return {"index": np.zeros((rows, 0), np.uint16), **{k: np.zeros((rows, 0), np.float32) for k in FIELDS[1:]}}
    wins = np.stack([x[r, w * hop:w * hop + step] for r in range(rows) for w in range(W)])
    got = dc.frames_metrics(O, wins, sf, osr, "raw", hann, dechirp, bw)
    return {k: got[k].reshape(rows, W) for k in FIELDS}


def find_frames_host(m, hop: int, sf: int, osr: int, frame_symbols: int, sync: int = 0x12, thresh_db: float = 0.0,
                     first: int = 0, row_len=None) -> np.ndarray:
    """The finder's rule on one row's scan (1-D arrays, or [1, W]); int64 starts."""
    N = 1 << sf
    step = N * osr
    assert 6 <= sf <= 12 and step % hop == 0 and step // hop >= 2
    k = step // hop
    sw0, sw1 = (sync >> 4) << (sf - 4), (sync & 15) << (sf - 4)
    frame_len = (frame_symbols + 2) * step
    index = np.asarray(m["index"]).reshape(-1).astype(np.int64)
    with np.errstate(invalid="ignore"):
        snr = np.asarray(m["power"], np.float32).reshape(-1) - np.asarray(m["power_avg"], np.float32).reshape(-1)
        ok = snr >= np.float32(thresh_db)  # NaN fails
    W = len(index)
    if row_len is None:
        row_len = (W - 1) * hop + step if W else 0
    starts = []
    w = -((-max(first - step // 2, 0)) // hop)
    while w < W - k:
        cand = ok[w] and ok[w + k] and (index[w + k] - index[w]) % N == (sw1 - sw0) % N
        d = (index[w] - sw0) % N
        if d >= N // 2:
            d -= N
        start = w * hop - d * osr
        if cand and start >= first and start + frame_len <= row_len:
            starts.append(start)
            first = start + frame_len
            w = max(w + 1, -((-(first - step // 2)) // hop))
        else:
            w += 1
    return np.array(starts, np.int64)


# (sf, osr, hop divisor k, data symbols, gaps before successive frames, sigma, sync)
TABLE = [
    (7, 1, 4, 6, (37, 5, 301, 900), 0.0, 0x12),
    (7, 1, 4, 6, (37, 5, 301, 900), 0.1, 0x12),
    (7, 1, 2, 6, (0, 1, 127, 64), 0.0, 0x12),
    (7, 1, 4, 6, (0, 0, 0, 1), 0.0, 0x12),
    (7, 1, 8, 6, (37, 5, 301, 900), 0.1, 0x12),
    (7, 1, 4, 6, (37, 5, 301, 900), 0.0, 0x34),
    (6, 1, 4, 6, (37, 5, 301, 90), 0.0, 0x12),
    (8, 1, 4, 20, (11, 77, 0, 513), 0.1, 0x12),
    (9, 1, 4, 3, (37, 5, 1301), 0.1, 0x12),
    (12, 1, 2, 1, (1000, 3), 0.0, 0x12),
    (7, 2, 4, 6, (36, 6, 300, 900), 0.0, 0x12),
    (10, 2, 4, 2, (38, 6), 0.0, 0x12),
]


def table_seed(ci: int) -> int:
    return 9100 + ci


def planted_layout(sf: int, osr: int, S: int, gaps):
    """(starts, total length) of frames of S data symbols, each after its gap."""
    frame_len = (S + 2) * (1 << sf) * osr
    starts, at = [], 0
    for g in gaps:
        at += g
        starts.append(at)
        at += frame_len
    return np.array(starts, np.int64), at


def planted_stream(O, sf: int, osr: int, S: int, gaps, sigma: float, sync: int, seed: int):
    """(stream complex64 [L], planted starts int64 [K], symbols uint16 [K, S]): oracle-modulated
    frames of random symbols written into zeros, then sigma * (normal + j normal) over all of it."""
    rng = np.random.default_rng(seed)
    starts, L = planted_layout(sf, osr, S, gaps)
    syms = rng.integers(0, 1 << sf, (len(gaps), S)).astype(np.uint16)
    x = np.zeros(L, np.complex64)
    frame_len = (S + 2) * (1 << sf) * osr
    for s, row in zip(starts, syms):
        x[s:s + frame_len] = O.lora_modulate(row, sf, osr, 125000, 1.0, sync)
    if sigma:
        x = (x + sigma * (rng.standard_normal(L) + 1j * rng.standard_normal(L))).astype(np.complex64)
    return x, starts, syms
