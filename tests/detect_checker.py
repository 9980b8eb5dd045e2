"""Host checker of the per-symbol detector metrics (tests only).

A numpy restatement of LoRaDetector<float>::detect (LoRaDetector.hpp:39-74) applied to
``Oracle().fft`` (the kissfft restatement) of a host-built window, and of the window each
mode feeds it: LEGACY (LoRaDemod.cpp:137-164), API (phy.cpp:197-227) and RAW (the bare
detector, oracle's orc_raw_demod).  Every fp32 operation is a separate numpy float32
operation in the reference's order; cosf / sinf / log10f / hypotf are the host libm's
(libm.so.6 through ctypes), as in the reference's x86-64 build; the detector's double
``total`` is the running sum in bin order (np.cumsum).

tests/golden/detect_metrics.json pins `detect` to the compiled reference header bit for bit;
the STRESS cases pin the window construction to the oracle's symbols.
"""
from __future__ import annotations

import ctypes as C
import ctypes.util
import math

import numpy as np

from tests.golden_inputs import cmul_f32, down_table

F32 = np.float32
PI_F = F32(3.14159265358979323846)
BW_SCALE = {125000: 1.0, 250000: 2.0, 500000: 4.0}

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _n in ("cosf", "sinf", "log10f"):
    getattr(_libm, _n).restype = C.c_float
    getattr(_libm, _n).argtypes = [C.c_float]
_libm.hypotf.restype = C.c_float
_libm.hypotf.argtypes = [C.c_float, C.c_float]


def _map(fn, x: np.ndarray) -> np.ndarray:
    return np.array([fn(float(v)) for v in x], F32)


def cscale(v: np.ndarray, w) -> np.ndarray:
    """std::complex<float> *= float: both components times w."""
    out = np.empty(v.shape, np.complex64)
    out.real = v.real.astype(F32) * w
    out.imag = v.imag.astype(F32) * w
    return out


def detect(X: np.ndarray):
    """(index, power, powerAvg, fIndex) of one spectrum, as LoRaDetector.hpp:43-73."""
    N = len(X)
    power_scale = F32(20 * math.log10(N))                     # :29
    re, im = X.real.astype(F32), X.imag.astype(F32)
    with np.errstate(all="ignore"):
        mag2 = re * re + im * im                              # :51, fp32, no contraction
        # strict '>' from maxValue = 0: the first maximum wins, NaN and 0 never do (:53-57)
        cand = np.where(mag2 > 0, mag2, F32(0))
        idx = int(np.argmax(cand))
        maxv = F32(cand[idx])
        total = np.cumsum(mag2.astype(np.float64))[-1]        # :45,52 double, bin order
        noise = np.sqrt(F32(total - np.float64(maxv)))        # :60
        fund = np.sqrt(maxv)                                  # :61
        pav = F32(20) * F32(_libm.log10f(float(noise))) - power_scale    # :63
        power = F32(20) * F32(_libm.log10f(float(fund))) - power_scale   # :64
        L, R = X[idx - 1 if idx > 0 else N - 1], X[idx + 1 if idx < N - 1 else 0]
        left = F32(_libm.hypotf(float(L.real), float(L.imag)))           # :66
        right = F32(_libm.hypotf(float(R.real), float(R.imag)))          # :67
        demon = 2.0 * np.float64(fund) - np.float64(right) - np.float64(left)   # :69
        fi = F32(0) if demon == 0.0 else F32(0.5 * np.float64(F32(right - left)) / demon)  # :70-71
    return idx, F32(power), F32(pav), F32(fi)


def round_to_int(x) -> int:
    """static_cast<int>(std::round(x)), saturating, NaN -> 0 (the C-ABI's stated rule)."""
    x = float(F32(x))
    if math.isnan(x):
        return 0
    r = math.copysign(math.floor(abs(x) + 0.5), x) if math.isfinite(x) else x
    return int(max(-2.0 ** 31, min(2.0 ** 31 - 1, r)))


def hann_window(N: int) -> np.ndarray:
    """LoRaDemod.cpp:19-21 / phy.cpp:39-41."""
    i = np.arange(N, dtype=F32)
    arg = F32(2.0) * PI_F * i / (F32(N) - F32(1.0))
    return F32(0.5) - F32(0.5) * _map(_libm.cosf, arg)


def frame_windows(M, x: np.ndarray, sf: int, osr: int = 1, mode: str = "legacy", hann: bool = False,
                  dechirp: bool = False, bw: int = 125000, cfo=0.0, time_offset=0.0, max_amp=0.0) -> np.ndarray:
    """The [total, N] FFT inputs of one frame, as the reference feeds them in `mode`."""
    N = 1 << sf
    step = N * osr
    x = np.ascontiguousarray(x, np.complex64)
    L = len(x)
    total = L // step
    out = np.zeros((total, N), np.complex64)
    if total == 0:
        return out
    down = down_table(M, sf, osr, BW_SCALE[bw]) if (dechirp and mode != "api") else None
    down1 = M.gen_chirp(N, 1, N, 0.0, True, 1.0, 0.0, BW_SCALE[bw])[0] if mode == "api" else None
    win = hann_window(N) if hann else None
    rot = mode != "raw"
    t_off = round_to_int(time_offset) if rot else 0
    rate = (F32(-2.0) * PI_F) * F32(cfo) / F32(N) if rot else F32(0)      # LoRaDemod.cpp:138
    i = np.arange(N)
    fi = i.astype(F32)
    for s in range(total):
        base = s * step                                                    # :142-149
        if t_off > 0:
            if base + t_off + step <= L:
                base += t_off
        elif t_off < 0:
            if -t_off <= base:
                base -= -t_off
        j = base + i * osr
        v = x[j]
        if mode == "api":
            v = cmul_f32(v, down1)                                         # phy.cpp:221
        else:
            if down is not None:
                v = cmul_f32(v, down[j % step])                            # e2e_chain_test.cpp:88-93
            if mode == "legacy" and F32(max_amp) > F32(1.0):
                v = cscale(v, F32(1.0) / F32(max_amp))                     # :68-77
        if rot:
            start = rate * (F32(s * N) + F32(t_off) / F32(osr))            # :151-152
            ph = start + rate * fi                                         # :154
            r = np.empty(N, np.complex64)
            r.real = _map(_libm.cosf, ph)
            r.imag = _map(_libm.sinf, ph)
            v = cmul_f32(v, r)                                             # :157-158
        if win is not None:
            v = cscale(v, win)                                             # :159-160
        out[s] = v
    return out


def frames_metrics(M, x2d: np.ndarray, sf: int, osr: int = 1, mode: str = "legacy", hann: bool = False,
                   dechirp: bool = False, bw: int = 125000, cfo=None, time_offset=None, max_amp=None):
    """detect() of every whole symbol of every frame of a [F, L] batch: a dict of [F, total]
    arrays (index uint16; power, power_avg, f_index float32)."""
    x2d = np.ascontiguousarray(x2d, np.complex64)
    F, L = x2d.shape
    total = L // ((1 << sf) * osr)
    res = {"index": np.zeros((F, total), np.uint16), "power": np.zeros((F, total), F32),
           "power_avg": np.zeros((F, total), F32), "f_index": np.zeros((F, total), F32)}
    for f in range(F):
        w = frame_windows(M, x2d[f], sf, osr, mode, hann, dechirp, bw,
                          0.0 if cfo is None else cfo[f], 0.0 if time_offset is None else time_offset[f],
                          0.0 if max_amp is None else max_amp[f])
        for s in range(total):
            idx, p, pav, fi = detect(M.fft(w[s]))
            res["index"][f, s], res["power"][f, s], res["power_avg"][f, s], res["f_index"][f, s] = idx, p, pav, fi
    return res


def bits(a) -> np.ndarray:
    """fp32 bit patterns (the comparisons are on these, so -inf, -0 and NaN count)."""
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---- the seeded windows of tests/golden/detect_metrics.json ------------------------------
GOLDEN_SFS = (6, 7, 8, 9, 10, 11, 12)
GOLDEN_SEED = 20251


def golden_windows(M, sf: int):
    """[(name, N-point complex64 window)] for one SF, from golden_inputs helpers and numpy
    PCG64 standard_normal only (no numpy transcendental on the path, so the sha256 recorded
    with each window holds on any host).  `M` modulates and generates chirps
    (oracle.pyoracle.Oracle)."""
    from tests.golden_inputs import dechirp

    N = 1 << sf
    rng = np.random.default_rng(GOLDEN_SEED + sf)

    def symbols(vals):
        """dechirped data-symbol windows of a noiseless frame carrying `vals`"""
        x = dechirp(M, M.lora_modulate(np.array(vals, np.uint16), sf, 1, 125000, 1.0, 0x12), sf)
        return x[2 * N:]

    def noisy(w, sigma):
        return (w + sigma * (rng.standard_normal(N) + 1j * rng.standard_normal(N))).astype(np.complex64)

    mid = N // 3
    clean = symbols([0, N - 1, mid])
    two = symbols([N // 5, (3 * N) // 4])
    alt = np.full(N, 0.5, np.complex64)
    alt[1::2] = -0.5
    wins = [
        ("clean_0", clean[:N]),                      # left neighbour wraps to bin N-1
        ("clean_last", clean[N:2 * N]),              # right neighbour wraps to bin 0
        ("clean_mid", clean[2 * N:3 * N]),
        ("two_tones", two[N // 3:N // 3 + N]),       # cut N/3 late across two symbols
        ("zero", np.zeros(N, np.complex64)),         # index 0, power -inf, powerAvg -inf
        ("constant", np.ones(N, np.complex64)),      # index 0, power 0 exactly, powerAvg -inf
        ("alternating", alt),                        # index N/2, power -6.0206, powerAvg -inf
        ("noise", noisy(np.zeros(N, np.complex64), 1.0)),
        ("tone_noise_1e-4", noisy(clean[2 * N:3 * N], 1e-4)),
        ("tone_noise_0.3", noisy(clean[2 * N:3 * N], 0.3)),
        ("tone_noise_2", noisy(clean[2 * N:3 * N], 2.0)),
        ("last_noise_0.05", noisy(clean[N:2 * N], 0.05)),
    ]
    return [(name, np.ascontiguousarray(w, np.complex64)) for name, w in wins]
