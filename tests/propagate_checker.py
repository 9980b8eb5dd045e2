"""The propagation stage's definition (include/lora_mi355x.h, lora_propagate_batch) restated in
numpy: the positions in int64, the tap sums and the path sums single float32 operations on
separate real and imaginary arrays in the header's order, the rotation's word in uint64 arithmetic
modulo 2^64 and its sine and cosine ``impair_checker``'s (glibc's own, one call per element).  It
does not import the library: the table is restated here too.  The GPU tests compare bits with it."""
import numpy as np

from tests.impair_checker import K, sincosf

F32 = np.float32
U64 = np.uint64
MAX_DELAY = 1 << 47
MAX_SFO = 1 << 20


def fracdelay_table(taps=16, beta=5.05) -> np.ndarray:
    """``stream.fracdelay_table``: [256, taps] float32, a Kaiser-windowed sinc in float64, rows
    normalised to sum 1 before the rounding, row 0 the unit impulse at taps/2 - 1."""
    half = taps // 2
    tab = np.zeros((256, taps), F32)
    for ph in range(256):
        u = np.arange(taps, dtype=np.float64) - (half - 1) - ph / 256.0
        z = 1.0 - (u / half) ** 2
        h = np.where(z >= 0.0, np.sinc(u) * np.i0(beta * np.sqrt(np.maximum(z, 0.0))) / np.i0(beta), 0.0)
        tab[ph] = (h / h.sum()).astype(F32)
    tab[0] = 0.0
    tab[0, half - 1] = 1.0
    return tab


def response_error(table, fmax=0.4, points=161) -> float:
    """max over the 256 phases and |f| <= fmax of |H_ph(f) - exp(-2 pi i f (taps/2 - 1 + ph/256))|,
    in float64, on ``points`` frequencies from -fmax to fmax."""
    tab = np.asarray(table, np.float64)
    T = tab.shape[1]
    f = np.linspace(-fmax, fmax, points)
    E = np.exp(-2j * np.pi * f[:, None] * np.arange(T)[None, :])            # [f, t]
    H = E @ tab.T                                                            # [f, ph]
    want = np.exp(-2j * np.pi * f[:, None] * (T // 2 - 1 + np.arange(256)[None, :] / 256.0))
    return float(np.abs(H - want).max())


def tri(n) -> np.ndarray:
    """n(n-1)/2 modulo 2^64 for uint64 ``n``: whichever of n, n-1 is even is halved, then the two
    are multiplied modulo 2^64."""
    n = np.asarray(n, U64)
    with np.errstate(over="ignore"):
        m = n - U64(1)
        odd = (n & U64(1)).astype(bool)
        return np.where(odd, n * (m >> U64(1)), (n >> U64(1)) * m)


def rotation_angle(n, fcw=0, rate=0, phase=0) -> np.ndarray:
    """th of samples ``n`` (uint64): (float)(int32)(W >> 32) * K."""
    n = np.asarray(n, U64)
    with np.errstate(over="ignore"):
        W = (U64((int(phase) & 0xFFFFFFFF) << 32) + U64(int(fcw) & (2 ** 64 - 1)) * n
             + U64(int(rate) & (2 ** 64 - 1)) * tri(n))
    return ((W >> U64(32)).astype(np.uint32).view(np.int32).astype(F32) * K).astype(F32)


def positions(n, delay: int, sfo: int, taps: int):
    """(j0, ph) of outputs ``n`` (int64) on one path."""
    m = -(np.int64(delay) + np.int64(sfo) * np.asarray(n, np.int64))
    q = m >> np.int64(32)
    ph = ((m & np.int64(0xFFFFFFFF)) >> np.int64(24)).astype(np.int64)
    return n + q - (taps // 2 - 1), ph


def _per_row(v, rows):
    if v is None:
        return None
    a = np.asarray(v, dtype=object).reshape(-1)
    return [int(a[0])] * rows if a.size == 1 else [int(x) for x in a]


def propagate_host(x, row_len=None, *, delay=0, gain=1.0, sfo=None, table=None, fcw=None, rate=None, phase=None,
                   in_first=0, first_sample=0) -> np.ndarray:
    """lora_propagate_batch's output for the complex64 rows ``x`` ([L] or [R, L]): complex64 [row_len]
    or [R, row_len].  ``delay`` (int words) and ``gain`` (complex) are a scalar, [P] or [R, P];
    ``sfo``, ``fcw``, ``rate`` (int words) and ``phase`` (an int32 word) None, a scalar or one per row."""
    x = np.asarray(x, np.complex64)
    one = x.ndim == 1
    x = x.reshape(1, -1) if one else x
    R, L = x.shape
    W = L if row_len is None else int(row_len)
    table = fracdelay_table() if table is None else np.asarray(table, F32)
    T = table.shape[1]
    d = np.asarray(delay, dtype=object)
    g = np.asarray(gain, np.complex64)
    d = d.reshape(1, -1) if d.ndim < 2 else d
    g = g.reshape(1, -1) if g.ndim < 2 else g
    P = max(d.shape[1], g.shape[1])
    d = np.broadcast_to(d, (R, P))
    g = np.broadcast_to(g, (R, P))
    so, fw, rt, ph0 = _per_row(sfo, R), _per_row(fcw, R), _per_row(rate, R), _per_row(phase, R)
    rot = fw is not None or rt is not None or ph0 is not None
    n = np.int64(first_sample) + np.arange(W, dtype=np.int64)
    t = np.arange(T, dtype=np.int64)
    out = np.empty((R, W), np.complex64)
    with np.errstate(all="ignore"):
        for r in range(R):
            re = np.ascontiguousarray(x[r].real, F32)
            im = np.ascontiguousarray(x[r].imag, F32)
            yr, yi = np.zeros(W, F32), np.zeros(W, F32)
            for p in range(P):
                dw, sw = int(d[r, p]), (0 if so is None else so[r])
                assert abs(dw) <= MAX_DELAY and abs(sw) <= MAX_SFO
                j0, ph = positions(n, dw, sw, T)
                sr, si = np.zeros(W, F32), np.zeros(W, F32)
                for k in range(T):
                    e = j0 + t[k] - np.int64(in_first)
                    ok = (e >= 0) & (e < L)
                    ec = np.where(ok, e, 0)
                    xr = np.where(ok, re[ec] if L else F32(0), F32(0)).astype(F32)
                    xi = np.where(ok, im[ec] if L else F32(0), F32(0)).astype(F32)
                    w = table[ph, k]
                    sr = (sr + (w * xr).astype(F32)).astype(F32)
                    si = (si + (w * xi).astype(F32)).astype(F32)
                gr, gi = F32(g[r, p].real), F32(g[r, p].imag)
                cr = ((gr * sr).astype(F32) - (gi * si).astype(F32)).astype(F32)
                ci = ((gr * si).astype(F32) + (gi * sr).astype(F32)).astype(F32)
                yr, yi = (yr + cr).astype(F32), (yi + ci).astype(F32)
            if rot:
                th = rotation_angle(n.astype(U64), 0 if fw is None else fw[r], 0 if rt is None else rt[r],
                                    0 if ph0 is None else ph0[r])
                s, c = sincosf(th)
                yr, yi = ((yr * c).astype(F32) - (yi * s).astype(F32)).astype(F32), \
                         ((yr * s).astype(F32) + (yi * c).astype(F32)).astype(F32)
            out[r].real, out[r].imag = yr, yi
    return out[0] if one else out


def delay_word(samples: float) -> int:
    """``stream.delay_word``: round(samples * 2^32) to nearest, ties to even."""
    return int(round(float(samples) * 4294967296.0))


def sfo_word(ppm: float) -> int:
    """``stream.sfo_word``: round(ppm * 1e-6 * 2^32) to nearest, ties to even."""
    return int(round(float(ppm) * 1e-6 * 4294967296.0))
