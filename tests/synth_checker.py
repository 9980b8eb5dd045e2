"""Host model of the wideband transmit side (tests only).

``synthesize_host``: the synthesis bank's definition (include/lora_mi355x.h,
lora_synthesize_batch) restated in numpy on separate fp32 real and imaginary arrays: every
product and every sum is its own float32 operation, rounded once, the taps of a phase
accumulated in a Python loop in order from +0.0, then the mix, then the channels in order from
+0.0.  numpy's complex multiplication is not used (its SIMD loops may fuse).
``synthesize_f64``: the direct zero-stuffed form - stuff, convolve, mix, sum - in float64, which
the roundings of the above are measured against.  ``store_host``: the raw store rule.
"""
from __future__ import annotations

import numpy as np

from tests import channel_checker as cc

F32 = np.float32

# numpy dtype -> (default inv_scale, bias, lo, hi, the code stored for NaN)
RAW = {np.dtype(np.int16): (32768.0, 0.0, -32768, 32767, 0),
       np.dtype(np.int8): (128.0, 0.0, -128, 127, 0),
       np.dtype(np.uint8): (127.5, 127.5, 0, 255, 128)}


def phases(ntaps: int, interp: int) -> int:
    """P = ceil(ntaps / interp): the taps of the longest phase."""
    return -(-ntaps // interp)


def outputs(chan_len: int, ntaps: int, interp: int) -> int:
    P = phases(ntaps, interp)
    return 0 if chan_len < P else (chan_len - P + 1) * interp


def delay(ntaps: int, interp: int) -> float:
    """Channel sample m is centred on output m * interp + delay."""
    return (ntaps - 1) / 2 - (phases(ntaps, interp) - 1) * interp


def nco_table(period: int):
    """(wr, wi) float32 [period]: exp(+2 pi i m / period), the conjugate of the banks' table."""
    wr, wi = cc.nco_table(period)
    return wr, -wi


def lowpass_taps(ntaps: int, cutoff: float, gain: float = 1.0) -> np.ndarray:
    """The formula of lora_phy_amd.stream.lowpass_taps with its gain, restated."""
    j = np.arange(ntaps, dtype=np.float64)
    h = 2 * cutoff * np.sinc(2 * cutoff * (j - (ntaps - 1) / 2)) * np.hamming(ntaps)
    h = h / h.sum()
    return (h if gain == 1.0 else h * gain).astype(F32)


def synthesize_host(chans, taps, interp: int, steps, period: int, gains=None, first_sample: int = 0,
                    nco=None) -> np.ndarray:
    """complex64 [W] for [C, Lc] channel streams, [R, W] for [R, C, Lc].  ``nco``: another (wr, wi)
    table than ``nco_table(period)`` (the table is an input of the C function)."""
    x = np.asarray(chans, np.complex64)
    h = np.asarray(taps, F32)
    T, U, C, Lc = len(h), int(interp), len(steps), x.shape[-1]
    assert x.shape[-2] == C
    g = np.ones(C, F32) if gains is None else np.asarray(gains, F32)
    P, W = phases(T, U), outputs(Lc, T, U)
    lead = x.shape[:-2]
    if W == 0:
        return np.zeros(lead + (0,), np.complex64)
    Q = W // U
    wr, wi = nco_table(period) if nco is None else (np.asarray(nco[0], F32), np.asarray(nco[1], F32))
    # (first_sample + t) mod period in Python integers: exact, non-negative
    pos = [(int(first_sample) + t) % period for t in range(W)]
    yr, yi = np.zeros(lead + (W,), F32), np.zeros(lead + (W,), F32)
    with np.errstate(all="ignore"):
        for c, k in enumerate(steps):
            ar = (g[c] * np.ascontiguousarray(x[..., c, :].real, F32)).astype(F32)
            ai = (g[c] * np.ascontiguousarray(x[..., c, :].imag, F32)).astype(F32)
            sr, si = np.zeros(lead + (W,), F32), np.zeros(lead + (W,), F32)
            for p in range(U):
                K = 0 if p >= T else -(-(T - p) // U)
                pr, pi = np.zeros(lead + (Q,), F32), np.zeros(lead + (Q,), F32)
                for i in range(K):
                    at = P - 1 - i  # output q of this phase meets sample q + P-1 - i
                    pr = pr + (h[p + i * U] * ar[..., at:at + Q]).astype(F32)
                    pi = pi + (h[p + i * U] * ai[..., at:at + Q]).astype(F32)
                sr[..., p::U], si[..., p::U] = pr, pi
            m = np.array([(int(k) * q) % period for q in pos], np.int64)
            zr = (sr * wr[m]).astype(F32) - (si * wi[m]).astype(F32)
            zi = (sr * wi[m]).astype(F32) + (si * wr[m]).astype(F32)
            yr = yr + zr
            yi = yi + zi
    out = np.zeros(lead + (W,), np.complex64)
    out.real, out.imag = yr, yi
    return out


def synthesize_f64(chans, taps, interp: int, steps, period: int, gains=None, first_sample: int = 0,
                   magnitudes: bool = False) -> np.ndarray:
    """The direct form in float64 (complex128 [W]) from the fp32 inputs and the fp32 table, for
    [C, Lc] streams: zero-stuff each gain-scaled channel by ``interp``, convolve it with the taps,
    keep the W "valid" outputs from (P - 1) * interp on, mix and sum.  ``magnitudes``: the same
    sums with every term replaced by an upper bound of its magnitude, |h| |g| (|xr| + |xi|) with
    the oscillator's components taken as 1 (float64 [W]): what a rounding bound scales with."""
    x = np.asarray(chans, np.complex64)
    h = np.asarray(taps, F32).astype(np.float64)
    T, U, C, Lc = len(h), int(interp), len(steps), x.shape[-1]
    g = (np.ones(C, F32) if gains is None else np.asarray(gains, F32)).astype(np.float64)
    P, W = phases(T, U), outputs(Lc, T, U)
    wr, wi = nco_table(period)
    w = wr.astype(np.float64) + 1j * wi.astype(np.float64)
    t = np.arange(W)
    out = np.zeros(W, np.float64 if magnitudes else np.complex128)
    if W == 0:
        return out
    for c, k in enumerate(steps):
        up = np.zeros(Lc * U, np.float64 if magnitudes else np.complex128)
        if magnitudes:
            up[::U] = abs(g[c]) * (np.abs(x[c].real.astype(np.float64)) + np.abs(x[c].imag.astype(np.float64)))
            out += np.convolve(np.abs(h), up)[(P - 1) * U:(P - 1) * U + W]
        else:
            up[::U] = g[c] * x[c].astype(np.complex128)
            s = np.convolve(h, up)[(P - 1) * U:(P - 1) * U + W]
            out += s * w[(int(k) * ((int(first_sample) + t) % period)) % period]
    return out


def store_host(y, dtype, inv_scale=None) -> np.ndarray:
    """The raw store rule: complex64 [..] to codes [.., 2] of ``dtype`` (int16, int8 or uint8).
    Per component v = y * inv_scale, for uint8 v = v + 127.5, each one fp32 operation;
    clamp(rint(v), lo, hi) with ties to even; a NaN v stores the format's zero."""
    dtype = np.dtype(dtype)
    default, bias, lo, hi, zero = RAW[dtype]
    s = F32(default if inv_scale is None else inv_scale)
    y = np.asarray(y, np.complex64)
    comp = np.stack([np.ascontiguousarray(y.real, F32), np.ascontiguousarray(y.imag, F32)], axis=-1)
    with np.errstate(all="ignore"):
        v = (comp * s).astype(F32)
        if bias:
            v = (v + F32(bias)).astype(F32)
        code = np.clip(np.rint(v), lo, hi)
    code = np.where(np.isnan(v), zero, code)
    return code.astype(np.int64).astype(dtype)


def planted_channels(O, ci: int):
    """(chans complex64 [C, L], planted) of ``channel_checker.CONFIGS[ci]``: the channel streams
    ``channel_checker.wideband`` builds its signal from, before its own upsampling -
    ``scan_checker.planted_stream`` of each TABLE row with sigma 0, seed SEED0 + c and sync 0x12,
    zero-extended by LEAD in front and to the longest plus PAD behind.  ``planted[c]`` = (starts
    in the extended channel's samples, symbols [K, S])."""
    from tests import scan_checker as sc

    rows = cc.CONFIGS[ci][6]
    chans, planted = [], []
    for c, ri in enumerate(rows):
        sf, osr, _, S, gaps, _, _ = sc.TABLE[ri]
        s, starts, syms = sc.planted_stream(O, sf, osr, S, gaps, 0.0, 0x12, cc.SEED0 + c)
        chans.append(s)
        planted.append((starts + cc.LEAD, syms))
    L = cc.LEAD + max(len(s) for s in chans) + cc.PAD
    out = np.zeros((len(chans), L), np.complex64)
    for c, s in enumerate(chans):
        out[c, cc.LEAD:cc.LEAD + len(s)] = s
    return out, planted


def loopback_shift(synth_taps: int, interp: int, chan_taps: int, decim: int) -> int:
    """How far a frame's start moves, in channel samples, through a synthesis bank and a
    down-converter bank at the same rate change: -(P-1) + (Ts-1)/(2U) - (Tc-1)/(2D), which the
    configurations used make a whole number."""
    from fractions import Fraction

    d = (-(phases(synth_taps, interp) - 1) + Fraction(synth_taps - 1, 2 * interp)
         - Fraction(chan_taps - 1, 2 * decim))
    assert d.denominator == 1, d
    return int(d)
