"""The payload codec on the GPU: symbols <-> bytes for whole batches of frames.

Torch-tensor wrappers over lora_decode_batch / lora_encode_batch / lora_decode_chain_batch /
lora_encode_chain_batch / lora_decode_chain_soft_batch (the chain decoder on per-bit LLRs)
(include/lora_mi355x.h, csrc/lora_codec.hip): one kernel per call on
the current torch stream, nothing leaves the device.  There is no CPU fallback (TypeError on
a CPU tensor); the host implementation of the same functions, :mod:`lora_phy_amd.codes`, is
the checker in the tests.

Symbols are uint16 tensors, payloads uint8 tensors, [F, n] or 1-D for a single frame.  Rows
may be strided views (unit stride within a row, rows not overlapping).

Self-describing frames (``encode_frame``, ``decode_header``, ``decode_frame`` over
lora_encode_frame_batch / lora_decode_frame_batch) put an explicit header in front of the chain:
the payload length, the coding rate and a CRC flag under the reference's 5-bit header checksum,
as five Hamming 8/4 codewords in a first block of eight symbols at rate 4/8 whose values are
multiples of four bins (a +-1 bin error is absorbed), and with the flag the SX1272 data checksum
of the whole payload behind it.  Rows of one batch may hold frames of different lengths and
coding rates; a decode needs no length from its caller.  The layout is this project's own (the
reference has the two checksums, no header), stated to the bit in include/lora_mi355x.h and
restated in numpy in tests/frame_checker.py.  SF 7-12.

``decode_header_soft`` and ``decode_frame_soft`` (lora_decode_frame_soft_batch) are the same two
decodes on per-bit LLRs whose header columns have the reduced form
(``DemodPlan.soft_bits(reduced=(2, 8))``): every codeword, the header's included, by maximum
likelihood, with a bound on the header bits the decoder may overrule; restated in
tests/frame_soft_checker.py.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

from . import _capi, codes
from .demod import _check_buf, _require_cuda, _stream_handle

MAX_PAYLOAD = 255  # bytes per frame of the encoders and the chain decoder

# the current stream's handle without building a torch.cuda.Stream object per call (a
# microsecond of the few a call costs on the host)
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(device: torch.device) -> int:
    return _raw_stream(device.index) if _raw_stream is not None else _stream_handle(device)


@dataclass
class DecodeResult:
    """Per-frame results of one decode call (all tensors on the symbols' device)."""

    payload: torch.Tensor            # [F, n] uint8
    crc_ok: Optional[torch.Tensor]   # [F] bool: the frame's last two bytes are its data checksum
    errors: torch.Tensor             # [F] int32: codewords whose decode flagged an error
    bad: Optional[torch.Tensor]      # [F] int32: uncorrectable Hamming 8/4 codewords (library decoder)


def _rows(t: torch.Tensor, name: str, dtype: torch.dtype):
    """-> (2-D view, squeeze): device, dtype and layout the C library cannot check."""
    _require_cuda(t, name)
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    squeeze = t.dim() == 1
    if squeeze:
        t = t.unsqueeze(0)
    if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        raise ValueError(f"{name} must be [frames, n] (or [n]) with unit stride within a row and "
                         "non-overlapping rows")
    return t, squeeze


def _row_stride(t: torch.Tensor) -> int:
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


def _symbols(t: torch.Tensor):
    if isinstance(t, torch.Tensor) and t.dtype in (torch.int16, torch.int32, torch.int64, torch.uint8):
        _require_cuda(t, "symbols")
        t = t.to(torch.int32).to(torch.uint16)  # the low 16 bits, as modulate() takes them
    return _rows(t, "symbols", torch.uint16)


def _out_rows(out: Optional[torch.Tensor], name: str, dtype: torch.dtype, F: int, n: int, squeeze: bool,
              device: torch.device) -> torch.Tensor:
    if out is None:
        return torch.empty((F, n), dtype=dtype, device=device)
    o, _ = _rows(out, name, dtype)
    if o.device != device or o.shape[0] != F or o.shape[1] != n or squeeze != (out.dim() == 1):
        raise ValueError(f"{name} must be a {dtype} {'[%d]' % n if squeeze else '[%d, %d]' % (F, n)} "
                         f"tensor on {device}")
    return o


def _ptr(t: torch.Tensor):
    return t.data_ptr() if t.numel() > 0 else None


def encode(payload: torch.Tensor, append_crc: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """lora_encode (LoRaEncoder.cpp:8-19): every byte -> two Hamming 8/4 codewords used as
    symbols, high nibble first.  ``append_crc``: the SX1272 data checksum of ``payload[2:]``
    follows as two more bytes (low byte first), so ``decode`` reports ``crc_ok``.
    Returns uint16 [F, 2 * (n + 2 * append_crc)]."""
    p, squeeze = _rows(payload, "payload", torch.uint8)
    F, n = p.shape
    if n > MAX_PAYLOAD:
        raise ValueError(f"payload rows hold at most {MAX_PAYLOAD} bytes")
    S = 2 * (n + (2 if append_crc else 0))
    o = _out_rows(out, "out", torch.uint16, F, S, squeeze, p.device)
    _capi.check(_capi.lib().lora_encode_batch(_ptr(p), F, n, _row_stride(p), int(bool(append_crc)), _ptr(o),
                                              _row_stride(o), p.device.index, _stream(p.device)))
    return o[0] if squeeze else o


def decode(symbols: torch.Tensor, out: Optional[DecodeResult] = None) -> DecodeResult:
    """lora_decode (LoRaDecoder.cpp:8-19) with the CRC check of lora_phy::decode
    (phy.cpp:241-256): pairs of symbols -> bytes through Hamming 8/4 on the symbols' low byte
    (an odd trailing symbol is ignored); per frame ``crc_ok``, and how many symbols flagged
    ``error`` / ``bad``.  ``out``: a DecodeResult of matching tensors to write into (no
    allocation)."""
    s, squeeze = _symbols(symbols)
    F, S = s.shape
    n = S // 2
    dev = s.device
    if out is None:
        out = DecodeResult(payload=torch.empty((n,) if squeeze else (F, n), dtype=torch.uint8, device=dev),
                           crc_ok=torch.empty(F, dtype=torch.bool, device=dev),
                           errors=torch.empty(F, dtype=torch.int32, device=dev),
                           bad=torch.empty(F, dtype=torch.int32, device=dev))
    pay = _out_rows(out.payload, "out.payload", torch.uint8, F, n, squeeze, dev)
    for name, dt in (("crc_ok", torch.bool), ("errors", torch.int32), ("bad", torch.int32)):
        _check_buf(getattr(out, name), "out." + name, dt, dev, F)
    _capi.check(_capi.lib().lora_decode_batch(_ptr(s), F, S, _row_stride(s), _ptr(pay), _row_stride(pay),
                                              out.crc_ok.data_ptr(), out.errors.data_ptr(), out.bad.data_ptr(),
                                              dev.index, _stream(dev)))
    return out


def chain_symbols(sf: int, cr, nbytes: int) -> int:
    """Symbols per frame of the chain for ``nbytes`` payload bytes (host arithmetic)."""
    return _capi.check(_capi.lib().lora_chain_symbols(int(sf), codes.rdd_of(cr), int(nbytes)))


def chain_capacity(sf: int, cr, nsymbols: int) -> int:
    """Payload bytes ``nsymbols`` symbols carry through the chain (whole blocks only)."""
    return min(MAX_PAYLOAD, nsymbols // (4 + codes.rdd_of(cr)) * int(sf) // 2)


def encode_chain(payload: torch.Tensor, sf: int, cr, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """codes.encode_chain on the device: nibbles -> codewords of rate 4/(4+RDD) (zero
    codewords pad to a multiple of sf) -> whitening -> diagonal interleave -> Gray.  ``cr``
    as codes.rdd_of takes it ('4/5'..'4/8', or RDD 0..4).  Returns uint16 [F, S]."""
    rdd = codes.rdd_of(cr)
    p, squeeze = _rows(payload, "payload", torch.uint8)
    F, n = p.shape
    lib = _capi.lib()
    S = _capi.check(lib.lora_chain_symbols(int(sf), rdd, n))
    o = _out_rows(out, "out", torch.uint16, F, S, squeeze, p.device)
    _capi.check(lib.lora_encode_chain_batch(int(sf), rdd, _ptr(p), F, n, _row_stride(p), _ptr(o), _row_stride(o),
                                            p.device.index, _stream(p.device)))
    return o[0] if squeeze else o


def decode_chain(symbols: torch.Tensor, sf: int, cr, nbytes: int, out: Optional[DecodeResult] = None) -> DecodeResult:
    """codes.decode_chain on the device: Gray -> diagonal deinterleave (whole blocks of 4+RDD
    symbols; trailing symbols are ignored) -> de-whitening -> nibble decode -> ``nbytes``
    bytes.  ``errors`` counts the codewords among the first 2 * nbytes that flagged an error;
    ``crc_ok`` and ``bad`` are None."""
    rdd = codes.rdd_of(cr)
    s, squeeze = _symbols(symbols)
    F, S = s.shape
    nbytes = int(nbytes)
    if not 0 <= nbytes <= MAX_PAYLOAD:
        raise ValueError(f"nbytes must be in 0..{MAX_PAYLOAD}")
    dev = s.device
    if out is None:
        out = DecodeResult(payload=torch.empty((nbytes,) if squeeze else (F, nbytes), dtype=torch.uint8,
                                               device=dev),
                           crc_ok=None, errors=torch.empty(F, dtype=torch.int32, device=dev), bad=None)
    pay = _out_rows(out.payload, "out.payload", torch.uint8, F, nbytes, squeeze, dev)
    _check_buf(out.errors, "out.errors", torch.int32, dev, F)
    _capi.check(_capi.lib().lora_decode_chain_batch(int(sf), rdd, _ptr(s), F, S, _row_stride(s), nbytes, _ptr(pay),
                                                    _row_stride(pay), out.errors.data_ptr(), dev.index,
                                                    _stream(dev)))
    return out


def decode_chain_soft(llr: torch.Tensor, sf: int, cr, nbytes: int, out: Optional[DecodeResult] = None) -> DecodeResult:
    """``decode_chain`` on per-bit LLRs (lora_decode_chain_soft_batch): ``llr`` is a float32
    [F, S, sf] (or [S, sf]) CUDA tensor as ``DemodPlan.soft_bits`` returns it, positive = 1;
    rows may be a view such as ``bits[:, 2:]`` (unit stride in the last dimension, pitch sf in
    the one before, rows not overlapping).  Deinterleaving and de-whitening act on the LLRs
    (a set whitening bit flips a sign); every codeword decodes to the nibble whose codeword
    correlates best with its 4 + RDD LLRs, the lowest nibble on a tie.  ``errors`` counts the
    codewords among the first 2 * nbytes whose chosen codeword differs from the signs of
    their LLRs; ``crc_ok`` and ``bad`` are None."""
    rdd = codes.rdd_of(cr)
    sf, nbytes = int(sf), int(nbytes)
    _require_cuda(llr, "llr")
    if llr.dtype != torch.float32:
        raise TypeError(f"llr must be torch.float32, got {llr.dtype}")
    squeeze = llr.dim() == 2
    t = llr.unsqueeze(0) if squeeze else llr
    if (t.dim() != 3 or t.shape[2] != sf or (sf > 1 and t.stride(2) != 1) or (t.shape[1] > 1 and t.stride(1) != sf)
            or (t.shape[0] > 1 and (t.stride(0) % sf or t.stride(0) < t.shape[1] * sf))):
        raise ValueError(f"llr must be [frames, symbols, {sf}] (or [symbols, {sf}]) with unit stride in the last "
                         f"dimension, pitch {sf} in the one before and non-overlapping rows")
    if not 0 <= nbytes <= MAX_PAYLOAD:
        raise ValueError(f"nbytes must be in 0..{MAX_PAYLOAD}")
    F, S = t.shape[0], t.shape[1]
    dev = t.device
    if out is None:
        out = DecodeResult(payload=torch.empty((nbytes,) if squeeze else (F, nbytes), dtype=torch.uint8,
                                               device=dev),
                           crc_ok=None, errors=torch.empty(F, dtype=torch.int32, device=dev), bad=None)
    pay = _out_rows(out.payload, "out.payload", torch.uint8, F, nbytes, squeeze, dev)
    _check_buf(out.errors, "out.errors", torch.int32, dev, F)
    _capi.check(_capi.lib().lora_decode_chain_soft_batch(sf, rdd, _ptr(t), F, S, t.stride(0) // sf if F > 1 else S,
                                                         nbytes, _ptr(pay), _row_stride(pay),
                                                         out.errors.data_ptr(), dev.index, _stream(dev)))
    return out


# ---------------------------------------------------------------------------------
# Self-describing frames (include/lora_mi355x.h, "Self-describing frames")
# ---------------------------------------------------------------------------------
FRAME_OK, FRAME_HEADER, FRAME_SHORT, FRAME_CRC = 0, 1, 2, 3
FRAME_MIN_SF = 7  # the header block carries sf - 7 data nibbles


@dataclass
class FrameResult:
    """Per-frame results of ``decode_frame`` / ``decode_header`` (int32 [F] tensors on the
    symbols' device).  ``status`` is FRAME_OK, FRAME_HEADER (bad header: every field 0),
    FRAME_SHORT (fewer than 8 symbols: every field 0; or fewer than the header's ``nsym``: the
    fields set, the payload zeros) or FRAME_CRC (the payload is written all the same)."""

    status: torch.Tensor
    nbytes: torch.Tensor             # payload bytes the header states
    rdd: torch.Tensor                # its coding rate, 4 / (4 + rdd)
    has_crc: torch.Tensor            # its CRC flag
    nsym: torch.Tensor               # data symbols of the whole frame
    errors: torch.Tensor             # header and data codewords whose decode flagged an error
    payload: Optional[torch.Tensor]  # [F, max_bytes] uint8, zeros beyond nbytes; None: header only
    # the soft decoders only: header bits in which the chosen codewords differ from the LLRs' signs
    hdr_flips: Optional[torch.Tensor] = None

    _FIELDS = ("status", "nbytes", "rdd", "has_crc", "nsym", "errors")


def frame_symbols(sf: int, cr, nbytes: int, crc: bool = True) -> int:
    """Data symbols of a self-describing frame of ``nbytes`` payload bytes: 8 of the header
    block, then ceil(K / sf) blocks of 4 + RDD with K = max(2 * (nbytes + 2 * crc) - (sf - 7), 0)
    (host arithmetic; SF 7-12)."""
    return _capi.check(_capi.lib().lora_frame_symbols(int(sf), codes.rdd_of(cr), int(nbytes), int(bool(crc))))


def frame_capacity(sf: int, nsymbols: int) -> int:
    """The most payload bytes a frame of ``nsymbols`` data symbols can state (rate 4/4, no
    CRC): the payload width ``decode_frame`` needs for rows of that many symbols."""
    if nsymbols < 8:
        return 0
    return min(MAX_PAYLOAD, ((nsymbols - 8) // 4 * int(sf) + int(sf) - FRAME_MIN_SF) // 2)


def _per_frame(t: Optional[torch.Tensor], name: str, F: int, device: torch.device):
    if t is None:
        return None
    _check_buf(t, name, torch.int32, device, F)
    if t.dim() != 1 or t.shape[0] != F:
        raise ValueError(f"{name} must be an int32 [{F}] tensor")
    return t.data_ptr() if F > 0 else None


def encode_frame(payload: torch.Tensor, nbytes: Optional[torch.Tensor], sf: int, cr, crc: bool = True,
                 out: Optional[torch.Tensor] = None, out_nsym: Optional[torch.Tensor] = None):
    """Self-describing frames on the device (lora_encode_frame_batch): ``payload`` is uint8
    [F, max_bytes] (or [max_bytes]), of which frame f uses ``nbytes[f]`` bytes (int32 [F] on the
    device, clamped to 0..max_bytes; None: max_bytes each).  The header states nbytes, the coding
    rate and the CRC flag; with ``crc`` the SX1272 data checksum of the whole payload follows it.
    Returns ``(symbols, nsym)``: uint16 [F, S] with S = frame_symbols(sf, cr, max_bytes, crc),
    zeros beyond each frame's own count, and that count, int32 [F]."""
    rdd = codes.rdd_of(cr)
    p, squeeze = _rows(payload, "payload", torch.uint8)
    F, n = p.shape
    lib = _capi.lib()
    S = _capi.check(lib.lora_frame_symbols(int(sf), rdd, n, int(bool(crc))))
    o = _out_rows(out, "out", torch.uint16, F, S, squeeze, p.device)
    if out_nsym is None:
        out_nsym = torch.empty(F, dtype=torch.int32, device=p.device)
    _capi.check(lib.lora_encode_frame_batch(int(sf), rdd, int(bool(crc)), _ptr(p), F, n, _row_stride(p),
                                            _per_frame(nbytes, "nbytes", F, p.device), _ptr(o), _row_stride(o),
                                            _per_frame(out_nsym, "out_nsym", F, p.device), p.device.index,
                                            _stream(p.device)))
    return (o[0] if squeeze else o), out_nsym


def _decode_frames(symbols, sf, avail, max_bytes, out, header_only):
    s, squeeze = _symbols(symbols)
    F, S = s.shape
    dev = s.device
    if header_only:
        max_bytes = 0
    elif max_bytes is None:
        max_bytes = frame_capacity(sf, S)
    max_bytes = int(max_bytes)
    if not 0 <= max_bytes <= MAX_PAYLOAD:
        raise ValueError(f"max_bytes must be in 0..{MAX_PAYLOAD}")
    if out is None:
        fields = {k: torch.empty(F, dtype=torch.int32, device=dev) for k in FrameResult._FIELDS}
        pay = None if header_only else torch.empty((max_bytes,) if squeeze else (F, max_bytes), dtype=torch.uint8,
                                                   device=dev)
        out = FrameResult(payload=pay, **fields)
    ptrs = [_per_frame(getattr(out, k), "out." + k, F, dev) for k in FrameResult._FIELDS]
    pay_ptr, pay_stride = None, 0
    if not header_only:
        # the library reads a NULL payload as header-only mode: a zero-width payload still has
        # a (never dereferenced) address of its own
        pay = _out_rows(out.payload, "out.payload", torch.uint8, F, max_bytes, squeeze, dev)
        pay_ptr, pay_stride = (pay.data_ptr() or out.status.data_ptr()), _row_stride(pay)
    _capi.check(_capi.lib().lora_decode_frame_batch(int(sf), _ptr(s), F, S, _row_stride(s),
                                                    _per_frame(avail, "avail", F, dev), *ptrs, pay_ptr,
                                                    max_bytes, pay_stride, dev.index, _stream(dev)))
    return out


def decode_header(symbols: torch.Tensor, sf: int, avail: Optional[torch.Tensor] = None,
                  out: Optional[FrameResult] = None) -> FrameResult:
    """The header of each row of ``symbols`` (uint16 [F, S] or [S]; only the first 8 are read):
    status FRAME_OK with nbytes, rdd, has_crc, nsym and the header's error count, FRAME_HEADER,
    or FRAME_SHORT when fewer than 8 symbols are there (``avail``: int32 [F] on the device,
    None: S each).  ``payload`` is None."""
    return _decode_frames(symbols, sf, avail, None, out, True)


def decode_frame(symbols: torch.Tensor, sf: int, avail: Optional[torch.Tensor] = None,
                 max_bytes: Optional[int] = None, out: Optional[FrameResult] = None) -> FrameResult:
    """Self-describing frames -> payloads (lora_decode_frame_batch): each row's header gives its
    length, coding rate and CRC flag, so rows of one batch may hold different frames.  ``avail``:
    how many of a row's S symbols belong to the frame (int32 [F] on the device, clamped to 0..S;
    None: S each).  ``max_bytes``: the payload's width, by default ``frame_capacity(sf, S)``, the
    most a frame of S symbols can hold (a frame stating more than max_bytes is FRAME_SHORT)."""
    return _decode_frames(symbols, sf, avail, max_bytes, out, False)


# ---------------------------------------------------------------------------------
# The same on soft bits (lora_decode_frame_soft_batch)
# ---------------------------------------------------------------------------------
MAX_HDR_FLIPS = 40  # the header's five codewords of eight bits


def _decode_frames_soft(llr, sf, avail, max_bytes, max_flips, out, header_only):
    sf, max_flips = int(sf), int(max_flips)
    _require_cuda(llr, "llr")
    if llr.dtype != torch.float32:
        raise TypeError(f"llr must be torch.float32, got {llr.dtype}")
    squeeze = llr.dim() == 2
    t = llr.unsqueeze(0) if squeeze else llr
    if (t.dim() != 3 or t.shape[2] != sf or (sf > 1 and t.stride(2) != 1) or (t.shape[1] > 1 and t.stride(1) != sf)
            or (t.shape[0] > 1 and (t.stride(0) % sf or t.stride(0) < t.shape[1] * sf))):
        raise ValueError(f"llr must be [frames, symbols, {sf}] (or [symbols, {sf}]) with unit stride in the last "
                         f"dimension, pitch {sf} in the one before and non-overlapping rows")
    if not 0 <= max_flips <= MAX_HDR_FLIPS:
        raise ValueError(f"max_flips must be in 0..{MAX_HDR_FLIPS}")
    F, S = t.shape[0], t.shape[1]
    dev = t.device
    if header_only:
        max_bytes = 0
    elif max_bytes is None:
        max_bytes = frame_capacity(sf, S)
    max_bytes = int(max_bytes)
    if not 0 <= max_bytes <= MAX_PAYLOAD:
        raise ValueError(f"max_bytes must be in 0..{MAX_PAYLOAD}")
    if out is None:
        fields = {k: torch.empty(F, dtype=torch.int32, device=dev) for k in FrameResult._FIELDS}
        pay = None if header_only else torch.empty((max_bytes,) if squeeze else (F, max_bytes), dtype=torch.uint8,
                                                   device=dev)
        out = FrameResult(payload=pay, hdr_flips=torch.empty(F, dtype=torch.int32, device=dev), **fields)
    ptrs = [_per_frame(getattr(out, k), "out." + k, F, dev) for k in FrameResult._FIELDS]
    flips = _per_frame(out.hdr_flips, "out.hdr_flips", F, dev)
    pay_ptr, pay_stride = None, 0
    if not header_only:
        # (a zero-width payload still has an address of its own, as in _decode_frames)
        pay = _out_rows(out.payload, "out.payload", torch.uint8, F, max_bytes, squeeze, dev)
        pay_ptr, pay_stride = (pay.data_ptr() or out.status.data_ptr()), _row_stride(pay)
    _capi.check(_capi.lib().lora_decode_frame_soft_batch(sf, _ptr(t), F, S, t.stride(0) // sf if F > 1 else S,
                                                         _per_frame(avail, "avail", F, dev), *ptrs, flips, max_flips,
                                                         pay_ptr, max_bytes, pay_stride, dev.index, _stream(dev)))
    return out


def decode_header_soft(llr: torch.Tensor, sf: int, avail: Optional[torch.Tensor] = None, max_flips: int = 5,
                       out: Optional[FrameResult] = None) -> FrameResult:
    """``decode_header`` on soft bits (lora_decode_frame_soft_batch, header-only mode): ``llr`` is
    a float32 [F, S, sf] (or [S, sf]) CUDA tensor, the DATA columns of each frame with the first
    eight in the reduced form - ``plan.soft_bits(iq, res, reduced=(2, 8))[:, 2:]``; rows may be
    such a view.  The five header codewords are decoded by maximum likelihood; ``errors`` counts
    those whose chosen codeword differs from the signs of their LLRs and ``hdr_flips`` the bit
    positions in which they do.  A header that needs more than ``max_flips`` (0 .. 40) of them is
    FRAME_HEADER, like one whose checksum or fields are wrong: the default 5 is what the hard
    gate tolerates (one bit in each codeword), and it is what keeps noise out.  ``payload`` is
    None."""
    return _decode_frames_soft(llr, sf, avail, None, max_flips, out, True)


def decode_frame_soft(llr: torch.Tensor, sf: int, avail: Optional[torch.Tensor] = None,
                      max_bytes: Optional[int] = None, max_flips: int = 5,
                      out: Optional[FrameResult] = None) -> FrameResult:
    """``decode_frame`` on soft bits (lora_decode_frame_soft_batch): the header as
    ``decode_header_soft`` reads it, then every data codeword by maximum likelihood at the header's
    coding rate, as ``decode_chain_soft`` decodes a chain.  ``avail`` and ``max_bytes`` as
    ``decode_frame``'s; the frame's CRC16 judges the soft decode (FRAME_CRC / FRAME_OK).
    ``errors`` counts the header and data codewords whose chosen codeword differs from the signs
    of their LLRs."""
    return _decode_frames_soft(llr, sf, avail, max_bytes, max_flips, out, False)
