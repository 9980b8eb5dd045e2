"""Host model of the rational-rate down-converter bank (tests only).

``resample_host``: the definition of lora_resample_channelize_batch (include/lora_mi355x.h)
restated in numpy on separate fp32 real and imaginary arrays, in the style of
``channel_checker.channelize_host``: every product and every sum is its own float32 operation,
rounded once, the taps of an output accumulated in a Python loop in order from +0.0, the zero
terms of the zero-stuffed stream left out.  ``resample_f64``: the direct form - zero-stuff,
filter, decimate - in double, which the polyphase indexing is measured against.
``wideband``: ``channel_checker.wideband`` for a wideband rate of decim / interp times the
channel rate.
"""
from __future__ import annotations

import numpy as np

from tests import channel_checker as cc
from tests import scan_checker as sc

F32 = np.float32


def outputs(row_len: int, ntaps: int, interp: int, decim: int) -> int:
    span = (row_len - 1) * interp + 1
    return 0 if row_len < 1 or span < ntaps else (span - ntaps) // decim + 1


def residue(r: int, ntaps: int, interp: int, decim: int):
    """(j0, off, K) of the outputs t = r + interp * u: the first tap, the first sample past
    u * decim, the number of taps."""
    j0 = (-(r * decim)) % interp
    off = (r * decim + j0) // interp
    K = 0 if j0 >= ntaps else -(-(ntaps - j0) // interp)
    return j0, off, K


def reach(ntaps: int, interp: int, decim: int) -> int:
    """The samples an output group u reaches from u * decim on: max over r of off + K."""
    return max(off + K for _, off, K in (residue(r, ntaps, interp, decim) for r in range(interp)))


def lowpass_taps(ntaps: int, cutoff: float, gain: float = 1.0) -> np.ndarray:
    """The formula of lora_phy_amd.stream.lowpass_taps, restated."""
    j = np.arange(ntaps, dtype=np.float64)
    h = 2 * cutoff * np.sinc(2 * cutoff * (j - (ntaps - 1) / 2)) * np.hamming(ntaps)
    return (h / h.sum() * gain).astype(F32)


def mixed(x, k: int, period: int, first_sample: int, wr, wi):
    """(zr, zi) float32: x times the oscillator of step k, four products, a difference, a sum."""
    xr, xi = np.ascontiguousarray(x.real, F32), np.ascontiguousarray(x.imag, F32)
    # (k * (first_sample + n)) mod period in Python integers: exact, non-negative
    m = np.array([(int(k) * ((int(first_sample) + n) % period)) % period for n in range(x.shape[-1])], np.int64)
    zr = (xr * wr[m]).astype(F32) - (xi * wi[m]).astype(F32)
    zi = (xr * wi[m]).astype(F32) + (xi * wr[m]).astype(F32)
    return zr, zi


def resample_host(x, taps, steps, period: int, interp: int, decim: int, first_sample: int = 0,
                  nco=None) -> np.ndarray:
    """complex64 [C, W] for a [L] input, [R, C, W] for [R, L]."""
    x = np.asarray(x, np.complex64)
    h = np.asarray(taps, F32)
    T, L, C = len(h), x.shape[-1], len(steps)
    W = outputs(L, T, interp, decim)
    out = np.zeros(x.shape[:-1] + (C, W), np.complex64)
    if W == 0:
        return out
    wr, wi = cc.nco_table(period) if nco is None else (np.asarray(nco[0], F32), np.asarray(nco[1], F32))
    with np.errstate(all="ignore"):
        for c, k in enumerate(steps):
            zr, zi = mixed(x, k, period, first_sample, wr, wi)
            for r in range(min(interp, W)):
                j0, off, K = residue(r, T, interp, decim)
                nu = (W - 1 - r) // interp + 1  # outputs r, r + interp, ..: u = 0 .. nu-1
                span = (nu - 1) * decim + 1
                yr = np.zeros(x.shape[:-1] + (nu,), F32)
                yi = np.zeros(x.shape[:-1] + (nu,), F32)
                for i in range(K):
                    yr = yr + (h[j0 + i * interp] * zr[..., off + i:off + i + span:decim]).astype(F32)
                    yi = yi + (h[j0 + i * interp] * zi[..., off + i:off + i + span:decim]).astype(F32)
                out[..., c, r::interp].real = yr
                out[..., c, r::interp].imag = yi
    return out


def resample_f64(x, taps, steps, period: int, interp: int, decim: int, first_sample: int = 0) -> np.ndarray:
    """The direct form in float64 (complex128 [C, W]) from the fp32 inputs and the fp32 table: the
    mixed stream zero-stuffed to ``interp`` times its length, and output t the dot product of all
    ``ntaps`` taps with the stuffed samples from t * decim on."""
    x = np.asarray(x, np.complex64).astype(np.complex128)
    h = np.asarray(taps, F32).astype(np.float64)
    T, L = len(h), x.shape[-1]
    W = outputs(L, T, interp, decim)
    wr, wi = cc.nco_table(period)
    w = wr.astype(np.float64) + 1j * wi.astype(np.float64)
    n = np.arange(L)
    out = np.zeros((len(steps), W), np.complex128)
    for c, k in enumerate(steps):
        z = x * w[(int(k) * ((int(first_sample) + n) % period)) % period]
        zup = np.zeros(max((L - 1) * interp + 1, 0), np.complex128)
        zup[::interp] = z
        for t in range(W):
            out[c, t] = np.dot(h, zup[t * decim:t * decim + T])
    return out


def wideband(O, rows, steps, amps, interp: int, decim: int, period: int, lead: int, pad: int, seed0: int,
             sigma: float, sync: int = 0x12):
    """``channel_checker.wideband`` at a wideband rate of decim / interp times the channel rate.
    The extended channels' common length Lc is padded to a multiple of ``interp``, and each is
    upsampled by band-limited FFT interpolation to ``Lw = Lc * decim // interp`` samples (the lower
    Lc // 2 bins first and the rest last in a zero spectrum of Lw bins, the inverse FFT times
    Lw / Lc, in double), then mixed up, summed, given noise and cast as there."""
    chans, planted = [], []
    for c, ri in enumerate(rows):
        sf, osr, _, S, gaps, _, _ = sc.TABLE[ri]
        s, starts, syms = sc.planted_stream(O, sf, osr, S, gaps, 0.0, sync, seed0 + c)
        chans.append(s)
        planted.append((starts + lead, syms))
    Lc = lead + max(len(s) for s in chans) + pad
    Lc += (-Lc) % interp
    Lw = Lc * decim // interp
    n = np.arange(Lw)
    x = np.zeros(Lw, np.complex128)
    for c, s in enumerate(chans):
        e = np.zeros(Lc, np.complex128)
        e[lead:lead + len(s)] = s
        X = np.fft.fft(e)
        Y = np.zeros(Lw, np.complex128)
        Y[:Lc // 2] = X[:Lc // 2]
        Y[Lw - (Lc - Lc // 2):] = X[Lc // 2:]
        up = np.fft.ifft(Y) * (Lw / Lc)
        x += amps[c] * up * np.exp(2j * np.pi * ((int(steps[c]) * n) % period) / period)
    if sigma:
        rng = np.random.default_rng(seed0 + 99)
        x = x + sigma * (rng.standard_normal(len(x)) + 1j * rng.standard_normal(len(x)))
    return x.astype(np.complex64), planted


# The end-to-end configurations: (sf, osr, interp, decim, period, ntaps, TABLE rows, steps, amps).
# The taps are lowpass_taps(ntaps, 0.5 / decim, gain=interp): the cutoff at the channel's edge.
CONFIGS = [
    (7, 1, 2, 5, 5, 41, (0, 2), (0, 2), (1, 1)),  # 2.5 channel widths of input: two adjacent channels
    (7, 1, 3, 8, 16, 49, (0, 2), (-4, 5), (1, 1)),
    (7, 1, 5, 96, 12, 385, (0, 2), (-2, 3), (1, 1)),
]
LEAD, PAD, SEED0 = 16, 64, 5000
SIGMAS = (0.0, 0.1)  # noiseless, and the integer bank's end-to-end noise level


def config_signal(O, ci: int, sigma: float):
    """(x, planted, taps) of configuration ci."""
    sf, osr, Li, D, period, T, rows, steps, amps = CONFIGS[ci]
    assert (T - 1) % (2 * D) == 0  # the delay, (T - 1) / (2 * D) channel samples, is a whole one
    x, planted = wideband(O, rows, steps, amps, Li, D, period, LEAD, PAD, SEED0, sigma)
    return x, planted, lowpass_taps(T, 0.5 / D, gain=Li)
