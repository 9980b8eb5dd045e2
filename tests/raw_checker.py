"""Host model of the raw sample conversion (tests only): include/lora_mi355x.h's
``x = ((float)v - bias) * scale`` in numpy fp32, every operation its own float32 operation.
The banks' models stay ``channel_checker.channelize_host`` and ``resample_checker.resample_host``,
applied to what ``to_cf32`` returns.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
# numpy dtype of a format: (bias, default scale before its rounding to fp32)
FORMATS = {np.dtype(np.int16): (0.0, 1.0 / 32768.0), np.dtype(np.int8): (0.0, 1.0 / 128.0),
           np.dtype(np.uint8): (127.5, 1.0 / 127.5)}


def default_scale(dtype) -> np.float32:
    return F32(FORMATS[np.dtype(dtype)][1])


def to_cf32(raw, scale=None) -> np.ndarray:
    """complex64 [..] of a raw [.., 2] array of int16, int8 or uint8 (I, Q)."""
    raw = np.asarray(raw)
    bias, _ = FORMATS[raw.dtype]
    assert raw.shape[-1] == 2
    scale = default_scale(raw.dtype) if scale is None else F32(scale)
    with np.errstate(all="ignore"):
        x = raw.astype(F32)
        if bias:
            x = x - F32(bias)
        x = (x * scale).astype(F32)
    out = np.empty(raw.shape[:-1], np.complex64)
    out.real, out.imag = x[..., 0], x[..., 1]
    return out
