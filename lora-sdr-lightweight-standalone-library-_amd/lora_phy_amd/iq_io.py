"""IQ file I/O: the reference runners' raw format, streamed into HBM.

Format (runners/rx_runner.cpp:72-79, runners/tx_runner.cpp:133-138): interleaved
little-endian float32 (I, Q) pairs, no header; a trailing unpaired float is ignored.
Files are memory-mapped and copied to the device in slices, so captures larger than
host RAM stream through; frames are rows of `frame_len` samples.

Raw SDR captures - interleaved integer (I, Q) pairs as the radios' tools write them: cs16
(little-endian int16), cs8, cu8 - are read the same way into [L, 2] integer tensors
(`read_raw`, `iter_stream_raw`), which `stream.Channelizer` takes as they are; `quantize` and
`write_raw` make such captures from complex64 samples.
"""
from __future__ import annotations

import os
from typing import Iterator, Optional, Tuple

import numpy as np
import torch


def _mmap(path: str) -> np.ndarray:
    n = os.path.getsize(path) // 8
    if n == 0:
        return np.zeros(0, np.complex64)
    return np.memmap(path, dtype=np.complex64, mode="r", shape=(n,))


def read_iq(path: str, device=None, frame_len: Optional[int] = None, max_samples: Optional[int] = None,
            slice_samples: int = 1 << 24) -> torch.Tensor:
    """Whole file (or its first `max_samples`) as complex64 on `device` ([L], or [F, frame_len]
    with the tail that does not fill a frame dropped, like rx_runner's whole-symbol rule)."""
    x = _mmap(path)
    if max_samples is not None:
        x = x[:max_samples]
    if frame_len:
        x = x[: (len(x) // frame_len) * frame_len]
    dev = torch.device("cpu") if device is None else torch.device(device)
    out = torch.empty(len(x), dtype=torch.complex64, device=dev)
    for s0 in range(0, len(x), slice_samples):
        part = torch.from_numpy(np.array(x[s0:s0 + slice_samples]))  # writable host copy
        out[s0:s0 + len(part)].copy_(part, non_blocking=False)
    return out.view(-1, frame_len) if frame_len else out


def iter_frames(path: str, frame_len: int, frames_per_chunk: int, device=None) -> Iterator[torch.Tensor]:
    """Stream a capture as [<=frames_per_chunk, frame_len] device tensors."""
    x = _mmap(path)
    nf = len(x) // frame_len
    dev = torch.device("cpu") if device is None else torch.device(device)
    for f0 in range(0, nf, frames_per_chunk):
        n = min(frames_per_chunk, nf - f0)
        host = np.array(x[f0 * frame_len:(f0 + n) * frame_len]).reshape(n, frame_len)
        yield torch.from_numpy(host).to(dev)


def iter_stream(path: str, chunk_samples: int, overlap: int, device=None) -> Iterator[Tuple[int, torch.Tensor]]:
    """Stream a capture as overlapping 1-D chunks: yields ``(offset, tensor)`` with
    ``tensor = file[offset : offset + chunk_samples + overlap]`` on ``device`` for offset = 0,
    chunk_samples, 2 * chunk_samples, ... while offset is inside the file.  Consecutive chunks
    share ``overlap`` samples; the last chunk, and only it, holds at most ``chunk_samples``.

    Receiving a continuous recording larger than HBM (``lora_phy_amd.stream``), with frames of
    ``frame_len = (frame_symbols + 2) * step`` samples: choose ``overlap >= frame_len + step``,
    so that a frame starting anywhere before ``chunk_samples`` lies whole in its chunk together
    with the windows that find it.  Per chunk, scan it and call ``find_frames`` with
    ``first = max(0, end_of_last_accepted_frame - offset)`` and ``row_len = len(tensor)``; in
    every chunk but the last, leave the starts at or beyond ``chunk_samples`` to the next
    chunk, which sees them again at ``start - chunk_samples``.  A frame's position in the file
    is ``offset + start`` and it ends at ``offset + start + frame_len``: every frame is found
    exactly once, whichever side of a chunk border it begins on."""
    chunk_samples, overlap = int(chunk_samples), int(overlap)
    if chunk_samples < 1 or overlap < 0:
        raise ValueError("chunk_samples must be >= 1 and overlap >= 0")
    x = _mmap(path)
    dev = torch.device("cpu") if device is None else torch.device(device)
    for off in range(0, len(x), chunk_samples):
        yield off, torch.from_numpy(np.array(x[off:off + chunk_samples + overlap])).to(dev)


def write_iq(path: str, iq: torch.Tensor) -> int:
    """tx_runner's output format; returns the number of samples written."""
    a = iq.detach().to("cpu").contiguous().view(-1).numpy().astype(np.complex64, copy=False)
    a.tofile(path)
    return len(a)


# ---- raw SDR captures: interleaved integer (I, Q) pairs, no header --------------------------
# torch.int16: cs16, little-endian (USRP, Pluto, LimeSDR, most .sigmf-data); torch.int8: cs8
# (HackRF); torch.uint8: cu8 (RTL-SDR).  In memory a capture is a [L, 2] tensor of that dtype
# (lora_phy_amd.stream's docstring has the conversion to fp32).
_RAW_NUMPY = {torch.int16: np.dtype("<i2"), torch.int8: np.dtype("i1"), torch.uint8: np.dtype("u1")}
# (bias, lowest code, highest code)
_RAW_RANGE = {torch.int16: (0.0, -32768, 32767), torch.int8: (0.0, -128, 127), torch.uint8: (127.5, 0, 255)}


def _raw_numpy(dtype) -> np.dtype:
    if dtype not in _RAW_NUMPY:
        raise TypeError(f"raw samples are torch.int16 (cs16), torch.int8 (cs8) or torch.uint8 (cu8), not {dtype}")
    return _RAW_NUMPY[dtype]


def _mmap_raw(path: str, dtype) -> np.ndarray:
    nd = _raw_numpy(dtype)
    n = os.path.getsize(path) // (2 * nd.itemsize)
    if n == 0:
        return np.zeros((0, 2), nd)
    return np.memmap(path, dtype=nd, mode="r", shape=(n, 2))


def _raw_tensor(part: np.ndarray, dtype) -> torch.Tensor:
    """A writable host copy of a slice of the map, in the machine's byte order."""
    return torch.from_numpy(np.array(part).astype(_raw_numpy(dtype).newbyteorder("="), copy=False))


def read_raw(path: str, dtype, device=None, max_samples: Optional[int] = None,
             slice_samples: int = 1 << 24) -> torch.Tensor:
    """Whole raw capture (or its first ``max_samples``) as a [L, 2] tensor of ``dtype`` on
    ``device``, memory-mapped and copied in slices like ``read_iq``; a trailing unpaired
    component is ignored."""
    x = _mmap_raw(path, dtype)
    if max_samples is not None:
        x = x[:max_samples]
    dev = torch.device("cpu") if device is None else torch.device(device)
    out = torch.empty((len(x), 2), dtype=dtype, device=dev)
    for s0 in range(0, len(x), slice_samples):
        part = _raw_tensor(x[s0:s0 + slice_samples], dtype)
        out[s0:s0 + len(part)].copy_(part, non_blocking=False)
    return out


def iter_stream_raw(path: str, dtype, chunk_samples: int, overlap: int,
                    device=None) -> Iterator[Tuple[int, torch.Tensor]]:
    """``iter_stream`` for a raw capture: yields ``(offset, tensor)`` with ``tensor = file[offset :
    offset + chunk_samples + overlap]`` as [.., 2] of ``dtype`` on ``device``, offsets and overlaps
    in complex samples and by ``iter_stream``'s contract."""
    chunk_samples, overlap = int(chunk_samples), int(overlap)
    if chunk_samples < 1 or overlap < 0:
        raise ValueError("chunk_samples must be >= 1 and overlap >= 0")
    x = _mmap_raw(path, dtype)
    dev = torch.device("cpu") if device is None else torch.device(device)
    for off in range(0, len(x), chunk_samples):
        yield off, _raw_tensor(x[off:off + chunk_samples + overlap], dtype).to(dev)


def quantize(iq: torch.Tensor, dtype, scale: Optional[float] = None) -> torch.Tensor:
    """complex64 [..] to raw samples [.., 2] of ``dtype`` on the same device, the inverse of
    ``stream.raw_to_complex``: per component ``q = clamp(rint(x / scale + bias), lo, hi)`` in fp32,
    ties to even, with the dtype's bias (127.5 for ``uint8``, else none) and code range and
    ``scale`` defaulting to ``stream.raw_scale(dtype)``.  How a test or a user makes a raw capture
    from ``LoRaMod`` output."""
    from .stream import raw_scale

    _raw_numpy(dtype)
    if iq.dtype != torch.complex64:
        raise TypeError("quantize takes complex64 samples")
    bias, lo, hi = _RAW_RANGE[dtype]
    scale = raw_scale(dtype) if scale is None else float(np.float32(scale))
    q = torch.view_as_real(iq) / scale
    if bias:
        q = q + bias
    return torch.clamp(torch.round(q), lo, hi).to(dtype)


def write_raw(path: str, raw: torch.Tensor) -> int:
    """Write a raw [L, 2] tensor (``int16`` little-endian, ``int8`` or ``uint8``) as the radios'
    tools do: interleaved I, Q, no header.  Returns the number of samples written."""
    nd = _raw_numpy(raw.dtype)
    if raw.dim() != 2 or raw.shape[1] != 2:
        raise ValueError("write_raw takes a [L, 2] tensor (I, Q)")
    raw.detach().to("cpu").contiguous().numpy().astype(nd, copy=False).tofile(path)
    return raw.shape[0]
