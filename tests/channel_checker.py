"""Host model of the wideband front end (tests only).

``channelize_host``: the down-converter bank's definition (include/lora_mi355x.h,
lora_channelize_batch) restated in numpy on separate fp32 real and imaginary arrays: every
product and every sum is its own float32 operation, rounded once, the taps accumulated in a
Python loop in order from +0.0.  numpy's complex multiplication is not used (its SIMD loops may
fuse).  ``wideband``: a test signal with one planted channel stream per channel, upsampled by
band-limited FFT interpolation and mixed up to its channel's centre.
"""
from __future__ import annotations

import numpy as np

from tests import scan_checker as sc

F32 = np.float32


def outputs(row_len: int, ntaps: int, decim: int) -> int:
    return 0 if row_len < ntaps else (row_len - ntaps) // decim + 1


def nco_table(period: int):
    """(wr, wi) float32 [period]: exp(-2 pi i m / period), cosine and sine in double, rounded."""
    ang = -2.0 * np.pi * np.arange(period, dtype=np.float64) / period
    return np.cos(ang).astype(F32), np.sin(ang).astype(F32)


def lowpass_taps(ntaps: int, cutoff: float) -> np.ndarray:
    """The formula of lora_phy_amd.stream.lowpass_taps, restated."""
    j = np.arange(ntaps, dtype=np.float64)
    h = 2 * cutoff * np.sinc(2 * cutoff * (j - (ntaps - 1) / 2)) * np.hamming(ntaps)
    return (h / h.sum()).astype(F32)


def channelize_host(x, taps, steps, period: int, decim: int, first_sample: int = 0, nco=None) -> np.ndarray:
    """complex64 [C, W] for a [L] input, [R, C, W] for [R, L].  ``nco``: another (wr, wi) table
    than ``nco_table(period)`` (the table is an input of the C function)."""
    x = np.asarray(x, np.complex64)
    xr, xi = np.ascontiguousarray(x.real, F32), np.ascontiguousarray(x.imag, F32)
    h = np.asarray(taps, F32)
    T, L, C = len(h), x.shape[-1], len(steps)
    W = outputs(L, T, decim)
    out = np.zeros(x.shape[:-1] + (C, W), np.complex64)
    if W == 0:
        return out
    wr, wi = nco_table(period) if nco is None else (np.asarray(nco[0], F32), np.asarray(nco[1], F32))
    # (k_c * (first_sample + n)) mod period in Python integers: exact, non-negative
    pos = [(int(first_sample) + n) % period for n in range(L)]
    span = (W - 1) * decim + 1
    with np.errstate(all="ignore"):
        for c, k in enumerate(steps):
            m = np.array([(int(k) * p) % period for p in pos], np.int64)
            zr = (xr * wr[m]).astype(F32) - (xi * wi[m]).astype(F32)
            zi = (xr * wi[m]).astype(F32) + (xi * wr[m]).astype(F32)
            yr = np.zeros(x.shape[:-1] + (W,), F32)
            yi = np.zeros(x.shape[:-1] + (W,), F32)
            for j in range(T):
                yr = yr + (h[j] * zr[..., j:j + span:decim]).astype(F32)
                yi = yi + (h[j] * zi[..., j:j + span:decim]).astype(F32)
            out[..., c, :].real = yr
            out[..., c, :].imag = yi
    return out


def channelize_f64(x, taps, steps, period: int, decim: int, first_sample: int = 0) -> np.ndarray:
    """The same sums evaluated directly in float64 (complex128 [C, W]) from the fp32 inputs and
    the fp32 table: what channelize_host's roundings are measured against."""
    x = np.asarray(x, np.complex64).astype(np.complex128)
    h = np.asarray(taps, F32).astype(np.float64)
    T, L = len(h), x.shape[-1]
    W = outputs(L, T, decim)
    wr, wi = nco_table(period)
    w = wr.astype(np.float64) + 1j * wi.astype(np.float64)
    n = np.arange(L)
    out = np.zeros((len(steps), W), np.complex128)
    for c, k in enumerate(steps):
        z = x * w[(int(k) * ((int(first_sample) + n) % period)) % period]
        for t in range(W):
            out[c, t] = np.dot(h, z[t * decim:t * decim + T])
    return out


def wideband(O, rows, steps, amps, decim: int, period: int, lead: int, pad: int, seed0: int, sigma: float,
             sync: int = 0x12):
    """(x complex64 [L * decim], planted): a wideband signal holding one channel per entry of
    ``rows``.  Channel c is ``scan_checker.planted_stream`` of ``TABLE[rows[c]]`` made with sigma 0
    and seed ``seed0 + c`` - and with ``sync``, since the wideband receiver takes one sync word for
    all channels - zero-extended by ``lead`` samples in front and to the longest channel plus
    ``pad`` behind (L samples in all).  It is upsampled by ``decim`` with band-limited FFT
    interpolation (the lower L // 2 bins first and the rest last in a zero spectrum of L * decim
    bins, the inverse FFT times decim, in double), multiplied by
    ``amps[c] * exp(+2 pi i ((k_c n) mod period) / period)`` and summed over the channels; then
    ``sigma * (normal + j normal)`` from ``default_rng(seed0 + 99)`` is added and the sum cast to
    complex64.  ``planted[c]`` = (starts in the extended channel's samples, symbols [K, S])."""
    chans, planted = [], []
    for c, ri in enumerate(rows):
        sf, osr, _, S, gaps, _, _ = sc.TABLE[ri]
        s, starts, syms = sc.planted_stream(O, sf, osr, S, gaps, 0.0, sync, seed0 + c)
        chans.append(s)
        planted.append((starts + lead, syms))
    L = lead + max(len(s) for s in chans) + pad
    n = np.arange(L * decim)
    x = np.zeros(L * decim, np.complex128)
    for c, s in enumerate(chans):
        e = np.zeros(L, np.complex128)
        e[lead:lead + len(s)] = s
        X = np.fft.fft(e)
        Y = np.zeros(L * decim, np.complex128)
        Y[:L // 2] = X[:L // 2]
        Y[L * decim - (L - L // 2):] = X[L // 2:]
        up = np.fft.ifft(Y) * decim
        x += amps[c] * up * np.exp(2j * np.pi * ((int(steps[c]) * n) % period) / period)
    if sigma:
        rng = np.random.default_rng(seed0 + 99)
        x = x + sigma * (rng.standard_normal(len(x)) + 1j * rng.standard_normal(len(x)))
    return x.astype(np.complex64), planted


# The end-to-end configurations: (sf, osr, decim, period, ntaps, cutoff, TABLE rows, steps, amps variants)
CONFIGS = [
    (7, 1, 8, 5, 65, 0.1, (0, 2, 3, 5, 1), (-2, -1, 0, 1, 2), ((1, 1, 1, 1, 1), (1, 0.1, 1, 0.1, 1))),
    (7, 2, 4, 5, 65, 0.2, (10, 10, 10), (-1, 0, 2), ((1, 1, 1),)),
    (8, 1, 8, 16, 65, 0.1, (7, 7), (-4, 5), ((1, 1), (1, 0.1))),
    (6, 1, 8, 5, 33, 0.1, (6, 6), (0, 2), ((1, 1), (1, 0.1))),
    (7, 1, 2, 8, 33, 0.3, (0,), (1,), ((1,),)),
    (9, 1, 4, 3, 33, 0.2, (8, 8), (-1, 1), ((1, 1),)),
]
LEAD, PAD, SEED0 = 16, 64, 4000


def config_signal(O, ci: int, ai: int, sigma: float):
    """(x, planted, taps) of configuration ci with its amps variant ai."""
    sf, osr, D, period, T, cutoff, rows, steps, amps = CONFIGS[ci]
    assert (T - 1) % (2 * D) == 0  # the delay is a whole channel sample
    x, planted = wideband(O, rows, steps, amps[ai], D, period, LEAD, PAD, SEED0, sigma)
    return x, planted, lowpass_taps(T, cutoff)
