"""The channel impairment stage's definition (include/lora_mi355x.h, lora_impair_batch) restated
in numpy: Philox4x32-10 in uint64 arithmetic, ``logf`` and ``sincosf`` glibc's own through ctypes
on libm.so.6 (one call per element: not ``np.log`` / ``np.sin``, whose SIMD paths are not glibc's,
and not csrc/lora_libm.h, which tests/test_libm_host.py pins to glibc on its own), ``sqrt``,
products and sums single numpy float32 operations on separate real and imaginary arrays, the raw
store ``synth_checker.store_host``.  The GPU tests compare bits with it."""
import ctypes as C
import ctypes.util

import numpy as np

from tests.synth_checker import store_host

F32 = np.float32
K = F32(float.fromhex("0x1.921fb6p-30"))  # fp32 pi * 2^-31
M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.logf.restype = C.c_float
_libm.logf.argtypes = [C.c_float]
_libm.sincosf.restype = None
_libm.sincosf.argtypes = [C.c_float, C.c_void_p, C.c_void_p]


def logf(x) -> np.ndarray:
    """glibc's logf of every element (float32 in, float32 out)."""
    x = np.ascontiguousarray(x, F32)
    f = _libm.logf
    return np.array([f(v) for v in x.ravel().tolist()], F32).reshape(x.shape)


def sincosf(x):
    """glibc's sincosf of every element: (sin, cos), float32."""
    x = np.ascontiguousarray(x, F32)
    s, c = np.empty(x.size, F32), np.empty(x.size, F32)
    ps, pc, f = s.ctypes.data, c.ctypes.data, _libm.sincosf
    for i, v in enumerate(x.ravel().tolist()):
        f(v, ps + 4 * i, pc + 4 * i)
    return s.reshape(x.shape), c.reshape(x.shape)


def philox4x32_10(counter, key) -> np.ndarray:
    """Philox4x32-10 of ``counter`` [.., 4] under ``key`` (2 words): [.., 4] uint32 words, all
    arithmetic in uint64."""
    c = [np.asarray(counter, np.uint64)[..., i] & MASK for i in range(4)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK,
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack(c, axis=-1).astype(np.uint32)


def noise_words(seed: int, R: int, n) -> tuple:
    """(w0, w1) of samples ``n`` (uint64 array) of row ``R``: words (0, 1) of block n >> 1 for an
    even n, words (2, 3) for an odd one."""
    n = np.asarray(n, np.uint64)
    b = n >> np.uint64(1)
    ctr = np.stack([b & MASK, b >> np.uint64(32), np.full_like(b, int(R) & 0xFFFFFFFF),
                    np.full_like(b, (int(R) >> 32) & 0xFFFFFFFF)], axis=-1)
    w = philox4x32_10(ctr, (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))
    odd = (n & np.uint64(1)).astype(bool)
    return np.where(odd, w[..., 2], w[..., 0]), np.where(odd, w[..., 3], w[..., 1])


def word_angle(p) -> np.ndarray:
    """(float)(int32)p * K for uint32 words p: one conversion, one product."""
    return (np.asarray(p, np.uint32).view(np.int32).astype(F32) * K).astype(F32)


def noise(seed: int, R: int, n, sigma):
    """(nr, ni) float32 of samples ``n`` of row ``R``."""
    w0, w1 = noise_words(seed, R, n)
    u = ((2 * (w0 >> np.uint32(9)).astype(np.int64) + 1).astype(F32) * F32(2.0 ** -24)).astype(F32)
    rad = np.sqrt((F32(-2.0) * logf(u)).astype(F32)).astype(F32)
    s, c = sincosf(word_angle(w1))
    a = (F32(sigma) * rad).astype(F32)
    return (a * c).astype(F32), (a * s).astype(F32)


def _per_row(v, rows, dtype):
    if v is None:
        return None
    a = np.asarray(v, dtype).reshape(-1)
    return np.broadcast_to(a, (rows,)) if a.size == 1 else a


def impair_host(x, rows=None, length=None, *, gain=None, fcw=None, phase=None, sigma=None, seed=0,
                first_sample=0, first_row=0) -> np.ndarray:
    """lora_impair_batch's output for the complex64 rows ``x`` ([L] or [R, L]; None: noise-only
    rows of ``rows`` x ``length``): complex64 of the same shape.  gain, fcw, phase and sigma are
    None (the stage is not performed), a scalar or one value per row."""
    if x is None:
        one, Rn, L = False, int(rows), int(length)
    else:
        x = np.asarray(x, np.complex64)
        one = x.ndim == 1
        x = x.reshape(1, -1) if one else x
        Rn, L = x.shape
    g, sg = _per_row(gain, Rn, F32), _per_row(sigma, Rn, F32)
    rot = x is not None and (fcw is not None or phase is not None)
    fw = _per_row(0 if fcw is None else fcw, Rn, np.int64)
    ph = _per_row(0 if phase is None else phase, Rn, np.int64)
    n = (np.uint64(int(first_sample)) + np.arange(L, dtype=np.uint64))
    out = np.empty((Rn, L), np.complex64)
    with np.errstate(all="ignore"):
        for r in range(Rn):
            yr = np.zeros(L, F32) if x is None else np.ascontiguousarray(x[r].real, F32)
            yi = np.zeros(L, F32) if x is None else np.ascontiguousarray(x[r].imag, F32)
            if x is not None and g is not None:
                yr, yi = (g[r] * yr).astype(F32), (g[r] * yi).astype(F32)
            if rot:
                p = ((int(ph[r]) & 0xFFFFFFFF) + (int(fw[r]) & 0xFFFFFFFF) * (n & MASK)) & MASK
                s, c = sincosf(word_angle(p.astype(np.uint32)))
                yr, yi = ((yr * c).astype(F32) - (yi * s).astype(F32)).astype(F32), \
                         ((yr * s).astype(F32) + (yi * c).astype(F32)).astype(F32)
            if sg is not None:
                nr, ni = noise(seed, int(first_row) + r, n, sg[r])
                if x is None:
                    yr, yi = nr, ni
                else:
                    yr, yi = (yr + nr).astype(F32), (yi + ni).astype(F32)
            out[r].real, out[r].imag = yr, yi
    return out[0] if one else out


def impair_raw_host(x, dtype, inv_scale=None, **kw) -> np.ndarray:
    """lora_impair_raw_batch: ``store_host`` of ``impair_host``."""
    return store_host(impair_host(x, **kw), dtype, inv_scale)


def cfo_word(cycles_per_sample: float) -> int:
    """``stream.cfo_word``: round(cycles * 2^32) to nearest, wrapped into int32."""
    w = int(round(float(cycles_per_sample) * 4294967296.0)) & 0xFFFFFFFF
    return w - (1 << 32) if w >= 1 << 31 else w
