"""Host model of preambled frames and their receive chain (tests only): the definitions of
include/lora_mi355x.h ("Preambled frames", the accumulating scan, the preamble finder, the
selection with a tail) restated in numpy on ``Oracle().fft`` and ``Oracle().gen_chirp``, as
tests/scan_checker.py restates the plain scan.

``tables_host`` / ``frame_host``: the frame on air.  ``scan_acc_host``: per-window |X|^2 spectra as
detect_checker builds and transforms them, summed in fp32 oldest first, then the detector's
statements on the sum.  ``find_preamble_host``: the rule, window by window.
``select_preamble_host``: the greedy pass with a tail and a carried word.  ``receive_host``: the
chain, with the oracle's demodulator, impair_checker's rotation and frame_checker's gate and decode.
"""
from __future__ import annotations

import numpy as np

from tests import detect_checker as dc
from tests import frame_checker as fc
from tests import impair_checker as ic
from tests import scan_checker as sc
from tests.golden_inputs import cmul_f32, down_table

F32 = np.float32


def tail_of(step: int) -> int:
    return 9 * step // 4


def tables_host(O, sf: int, osr: int = 1, preamble: int = 8, bw: int = 125000, amplitude: float = 1.0):
    """(pre, sfd): ``preamble`` up-chirps and two and a quarter down-chirps, each chain from phase 0
    with the phase carried (ChirpGenerator.hpp:23-50), the amplitude clamped as lora_modulate's."""
    N = 1 << sf
    step = N * osr
    bws = dc.BW_SCALE[bw]
    ampl = float(max(-1.0, min(1.0, amplitude)))
    ph, parts = 0.0, []
    for _ in range(preamble):
        c, ph = O.gen_chirp(N, osr, step, 0.0, False, ampl, ph, bws)
        parts.append(c)
    pre = np.concatenate(parts)
    ph, parts = 0.0, []
    for nn in (step, step, step // 4):
        c, ph = O.gen_chirp(N, osr, nn, 0.0, True, ampl, ph, bws)
        parts.append(c)
    return pre, np.concatenate(parts)


def frame_host(O, syms, sf: int, osr: int = 1, preamble: int = 8, sync: int = 0x12, bw: int = 125000,
               amplitude: float = 1.0) -> np.ndarray:
    """[pre | sync | sfd | data] of one frame."""
    step = (1 << sf) * osr
    f = O.lora_modulate(np.asarray(syms, np.uint16), sf, osr, bw, amplitude, sync)
    pre, sfd = tables_host(O, sf, osr, preamble, bw, amplitude)
    return np.concatenate([pre, f[:2 * step], sfd, f[2 * step:]]).astype(np.complex64)


def gather_sync_data(x, start: int, step: int, data_len: int, cut: int) -> np.ndarray:
    """What the chain cuts for a slot: 2 * step samples at start, data_len at start + 2 * step +
    tail, zeros up to cut."""
    out = np.zeros(cut, np.complex64)
    if start < 0:
        return out
    out[:2 * step] = fc.gather_host(x, [start], [2 * step], 2 * step)[0]
    out[2 * step:] = fc.gather_host(x, [start + 2 * step + tail_of(step)], [data_len], cut - 2 * step)[0]
    return out


# ---- the accumulating scan ---------------------------------------------------------------------
def window_spectra(O, x, sf: int, osr: int, hop: int, conj: bool = False, hann: bool = False,
                   dechirp: bool = True, bw: int = 125000) -> np.ndarray:
    """float32 [W, N]: re*re + im*im of every plain window's spectrum (LoRaDetector.hpp:51)."""
    x = np.ascontiguousarray(x, np.complex64)
    N = 1 << sf
    step = N * osr
    W = sc.scan_windows(len(x), step, hop)
    out = np.zeros((W, N), F32)
    if W == 0:
        return out
    if conj:
        x = np.conj(x)
    i = np.arange(N) * osr
    down = down_table(O, sf, osr, dc.BW_SCALE[bw])[i] if dechirp else None
    win = dc.hann_window(N) if hann else None
    with np.errstate(all="ignore"):
        for w in range(W):
            v = x[w * hop + i]
            if down is not None:
                v = cmul_f32(v, down)
            if win is not None:
                v = dc.cscale(v, win)
            X = O.fft(v)
            re, im = X.real.astype(F32), X.imag.astype(F32)
            out[w] = re * re + im * im
    return out


def detect_sum(S: np.ndarray):
    """(index, power, power_avg) of one summed spectrum: LoRaDetector.hpp:43-64 on S."""
    N = len(S)
    power_scale = F32(20 * np.log10(N))
    with np.errstate(all="ignore"):
        cand = np.where(S > 0, S, F32(0))
        idx = int(np.argmax(cand))
        maxv = F32(cand[idx])
        total = np.cumsum(S.astype(np.float64))[-1]
        noise = np.sqrt(F32(total - np.float64(maxv)))
        fund = np.sqrt(maxv)
        pav = F32(20) * F32(dc._libm.log10f(float(noise))) - power_scale
        power = F32(20) * F32(dc._libm.log10f(float(fund))) - power_scale
    return idx, F32(power), F32(pav)


def scan_acc_windows(row_len: int, step: int, hop: int, acc: int) -> int:
    W = sc.scan_windows(row_len, step, hop)
    return W if acc <= 1 else max(W - (acc - 1) * (step // hop), 0)


def scan_acc_host(O, x, sf: int, osr: int = 1, hop: int = 1, acc: int = 1, conj: bool = False, hann: bool = False,
                  dechirp: bool = True, bw: int = 125000):
    """dict of [rows, Wa] arrays (index uint16; power, power_avg float32) for a [L] or [rows, L]
    stream."""
    x = np.ascontiguousarray(x, np.complex64)
    if x.ndim == 1:
        x = x[None]
    rows, L = x.shape
    step = (1 << sf) * osr
    assert 1 <= acc <= 8 and (acc == 1 or step % hop == 0)
    k = step // hop if acc > 1 else 0
    Wa = scan_acc_windows(L, step, hop, acc)
    out = {"index": np.zeros((rows, Wa), np.uint16), "power": np.zeros((rows, Wa), F32),
           "power_avg": np.zeros((rows, Wa), F32)}
    if Wa == 0:
        return out
    for r in range(rows):
        P = window_spectra(O, x[r], sf, osr, hop, conj, hann, dechirp, bw)
        for w in range(Wa):
            S = P[w]
            for q in range(1, acc):
                S = (S + P[w + q * k]).astype(F32)  # one rounding per addition, oldest first
            out["index"][r, w], out["power"][r, w], out["power_avg"][r, w] = detect_sum(S)
    return out


# ---- the finder and the selection ----------------------------------------------------------------
def centred(v: int, N: int) -> int:
    v %= N
    return v - N if v >= N // 2 else v


def find_preamble_host(up, dn, hop: int, sf: int, osr: int, m: int, thresh_up_db: float = 0.0,
                       thresh_dn_db: float = 0.0, max_cfo_bins=None, row_len=None):
    """Every (start, c) one row lists (1-D arrays, or [1, W]), uncut by any capacity: int64 [K, 2]."""
    N = 1 << sf
    step = N * osr
    assert 7 <= sf <= 12 and step % hop == 0 and step // hop >= 4 and 2 <= m <= 8
    k = step // hop
    max_cfo_bins = N // 4 - 1 if max_cfo_bins is None else max_cfo_bins
    tail = tail_of(step)
    ui = np.asarray(up["index"]).reshape(-1).astype(np.int64)
    di = np.asarray(dn["index"]).reshape(-1).astype(np.int64)
    dp = np.asarray(dn["power"], F32).reshape(-1)
    with np.errstate(invalid="ignore"):
        usnr = np.asarray(up["power"], F32).reshape(-1) - np.asarray(up["power_avg"], F32).reshape(-1)
        dsnr = dp - np.asarray(dn["power_avg"], F32).reshape(-1)
        uok, dok = usnr >= F32(thresh_up_db), dsnr >= F32(thresh_dn_db)  # NaN fails
    Wu, Wd = len(ui), len(di)
    if row_len is None:
        row_len = (Wd - 1) * hop + 2 * step if Wd else 0
    out, prev = [], None
    lag = (2 + m) * k
    for w in range(lag, Wd - k):
        u = w - lag
        if u >= Wu:
            break
        with np.errstate(invalid="ignore"):
            if not (dok[w] and uok[u] and dp[w] >= dp[w - k] and dp[w] > dp[w + k]):
                continue
        s = centred(int(ui[u] + di[w]), N)
        d = s // 2  # floor
        c = centred(int(ui[u]) - d, N)
        start = w * hop - d * osr - 2 * step
        if abs(c) > max_cfo_bins or start < 0 or start + 10 * step + tail > row_len:
            continue
        if prev != (start, c):
            out.append((start, c))
        prev = (start, c)
    return np.array(out, np.int64).reshape(-1, 2)


def select_preamble_host(starts, words, status, nsym, step: int, tail: int, row_len: int, max_symbols: int,
                         first: int = 0):
    """The greedy pass over one row's slots, in slot order -> (accepted starts int64, their words
    int32, their nsym int32, end), uncut by any capacity."""
    out, outw, outn = [], [], []
    for s, wd, st, n in zip(starts, words, status, nsym):
        s, n = int(s), int(n)
        if st == fc.OK and 0 <= n <= max_symbols and s >= 0 and s >= first and s + (2 + n) * step + tail <= row_len:
            out.append(s)
            outw.append(int(wd))
            outn.append(n)
            first = s + (2 + n) * step + tail
    return np.array(out, np.int64), np.array(outw, np.int32), np.array(outn, np.int32), first


def derotation_word(c: int, step: int) -> int:
    """floor(-c * 2^32 / step) wrapped into int32."""
    w = ((-int(c) << 32) // int(step)) & 0xFFFFFFFF
    return w - (1 << 32) if w >= 1 << 31 else w


def receive_host(O, x, sf: int, osr: int, max_symbols: int, hop: int, m: int = 6, thresh_up_db: float = 0.0,
                 thresh_dn_db: float = 0.0, max_cfo_bins=None, first: int = 0, cand_capacity=None,
                 max_bytes: int = fc.MAX_PAYLOAD, soft: bool = False, max_flips: int = 5):
    """stream.receive_preamble_frames_device on one row, on the CPU -> dict: candidates ([K, 2]
    start, c), starts, cfo_bins, nsym, end, and per accepted frame frame_checker's decode (or
    frame_soft_checker's) plus the demodulated symbols, sync, cfo, time_offset."""
    from tests import frame_soft_checker as fsc

    x = np.ascontiguousarray(x, np.complex64)
    step = (1 << sf) * osr
    tail = tail_of(step)
    L = len(x)
    up = scan_acc_host(O, x, sf, osr, hop, m)
    dn = scan_acc_host(O, x, sf, osr, hop, 2, conj=True)
    cands = find_preamble_host(up, dn, hop, sf, osr, m, thresh_up_db, thresh_dn_db, max_cfo_bins, L)
    cap = -(-L // (4 * step)) if cand_capacity is None else cand_capacity
    kept = cands[:cap]

    def cut(starts, cfo, data_len, n):
        rows = np.stack([gather_sync_data(x, int(s), step, int(dl), n) for s, dl in zip(starts, data_len)])
        return ic.impair_host(rows, fcw=[derotation_word(c, step) for c in cfo])

    def demod(rows):
        syms, sy, cfo, toff, cnt = O.demod_frames(rows, sf, osr, False, True)
        llr = None
        if soft:
            amp = np.array([fsc.max_amplitude(O, r, sf, osr) for r in rows], F32)
            llr = fsc.soft_bits_frames(O, rows, sf, osr, "legacy", False, True, 125000, cfo, toff, amp, (2, 8))
        return syms, sy, cfo, toff, cnt, llr

    status, hsym = np.zeros(len(kept), np.int32), np.zeros(len(kept), np.int32)
    if len(kept):
        heads = cut(kept[:, 0], kept[:, 1], [8 * step] * len(kept), 10 * step)
        syms, _, _, _, cnt, llr = demod(heads)
        for j in range(len(kept)):
            h = fsc.decode_header_soft(llr[j, 2:], sf, None, max_flips) if soft else fc.decode_header(syms[j, :cnt[j]], sf)
            status[j], hsym[j] = h["status"], h["nsym"]
    starts, cfo_bins, nsym, end = select_preamble_host(kept[:, 0], kept[:, 1], status, hsym, step, tail, L,
                                                       max_symbols, first)
    out = {"candidates": cands, "starts": starts, "cfo_bins": cfo_bins, "nsym": nsym, "end": end, "frames": []}
    if len(starts):
        frames = cut(starts, cfo_bins, nsym.astype(np.int64) * step, (2 + max_symbols) * step)
        syms, sy, cfo, toff, cnt, llr = demod(frames)
        for j in range(len(starts)):
            if soft:
                f = fsc.decode_frame_soft(llr[j, 2:], sf, int(nsym[j]), max_bytes, max_flips)
            else:
                f = fc.decode_frame(syms[j, :cnt[j]], sf, int(nsym[j]), max_bytes)
            f.update(symbols=syms[j, :cnt[j]].copy(), sync=sy[j], cfo=cfo[j], time_offset=toff[j])
            out["frames"].append(f)
    return out


# ---- the table -----------------------------------------------------------------------------------
# (sf, osr, hop divisor k, preamble P, acc m, data symbols, gaps before successive frames, sigma,
#  carrier offset in bins)
TABLE = [
    (7, 1, 4, 8, 6, 10, (300, 0, 77), 0.0, 0.0),
    (7, 1, 4, 8, 6, 10, (300, 0, 77), 0.1, 5.0),
    (7, 1, 4, 8, 6, 10, (300, 5, 901), 0.1, -9.25),
    (7, 1, 8, 8, 6, 10, (37, 5, 301), 0.1, 3.25),
    (7, 1, 4, 8, 6, 10, (0, 1, 127), 0.0, 31.0),
    (7, 2, 4, 8, 6, 10, (36, 6, 300), 0.02, 4.0),
    (8, 1, 4, 6, 4, 12, (11, 77, 0), 0.1, -30.0),
    (9, 1, 4, 8, 6, 9, (37, 1301), 0.1, -20.4),
    (10, 2, 4, 8, 6, 8, (38,), 0.0, 7.0),
    (12, 1, 4, 8, 6, 8, (1000,), 0.0, 100.0),
]


def table_seed(ci: int) -> int:
    return 9300 + ci


def apply_cfo(x: np.ndarray, cfo_bins: float, step: int) -> np.ndarray:
    """x[n] * exp(2 pi j cfo n / step), computed in double."""
    if not cfo_bins:
        return np.ascontiguousarray(x, np.complex64)
    n = np.arange(len(x), dtype=np.float64)
    return (x.astype(np.complex128) * np.exp(2j * np.pi * cfo_bins * n / step)).astype(np.complex64)


def plant(O, frames, sf: int, osr: int, gaps, sigma: float, cfo: float, rng) -> tuple:
    """(stream, starts): the given preambled frames (each with its count of preamble samples) written
    into zeros, each after its gap, a trailing step of zeros, the carrier offset over all of it and
    then sigma * (normal + j normal).  starts: each frame's first sync symbol."""
    step = (1 << sf) * osr
    at, starts, parts = 0, [], []
    for g, (f, pre_len) in zip(gaps, frames):
        parts.append(np.zeros(g, np.complex64))
        at += g
        starts.append(at + pre_len)
        parts.append(f)
        at += len(f)
    parts.append(np.zeros(step, np.complex64))
    x = apply_cfo(np.concatenate(parts), cfo, step)
    if sigma:
        L = len(x)
        x = (x + sigma * (rng.standard_normal(L) + 1j * rng.standard_normal(L))).astype(np.complex64)
    return x, np.array(starts, np.int64)


def planted_stream(O, ci: int):
    """(stream complex64 [L], planted (start, round(cfo)) int64 [K, 2], symbols uint16 [K, S]) of
    table case ci: frames of random data symbols."""
    sf, osr, k, P, m, S, gaps, sigma, cfo = TABLE[ci]
    rng = np.random.default_rng(table_seed(ci))
    step = (1 << sf) * osr
    syms = rng.integers(0, 1 << sf, (len(gaps), S)).astype(np.uint16)
    frames = [(frame_host(O, row, sf, osr, P), P * step) for row in syms]
    x, starts = plant(O, frames, sf, osr, gaps, sigma, cfo, rng)
    want = np.stack([starts, np.full(len(starts), int(round(cfo)), np.int64)], axis=1)
    return x, want, syms


def packet_stream(O, ci: int, rdds=(1, 4, 2), crcs=(1, 0, 1)):
    """Table case ci with self-describing frames of mixed payload lengths, coding rates and CRC
    flags instead of random symbols -> (stream, planted [K, 2], payloads list of bytes, max_symbols)."""
    sf, osr, k, P, m, S, gaps, sigma, cfo = TABLE[ci]
    rng = np.random.default_rng(table_seed(ci) + 50)
    step = (1 << sf) * osr
    frames, payloads, longest = [], [], 8
    for j in range(len(gaps)):
        n = int(rng.integers(0, 7))
        pl = bytes(rng.integers(0, 256, n, dtype=np.uint8).tolist())
        syms = fc.encode_frame(pl, sf, rdds[j % len(rdds)], crcs[j % len(crcs)])
        longest = max(longest, len(syms))
        payloads.append(pl)
        frames.append((frame_host(O, syms, sf, osr, P), P * step))
    x, starts = plant(O, frames, sf, osr, gaps, sigma, cfo, rng)
    want = np.stack([starts, np.full(len(starts), int(round(cfo)), np.int64)], axis=1)
    return x, want, payloads, longest
