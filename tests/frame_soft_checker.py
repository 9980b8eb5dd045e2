"""Host checker of the soft path through the self-describing frame (tests only).

A numpy restatement of two definitions in include/lora_mi355x.h, on top of tests/soft_checker.py,
tests/frame_checker.py and lora_phy_amd.codes:

* ``soft_bits_reduced`` - a reduced column of lora_demod_soft_bits_frame_batch: the LLRs of the
  sf - 2 bits of grayToBinary16(((k + 2) >> 2) & (2^(sf-2) - 1)), the value the frame's header
  block carries, then two +0.0.  ``soft_bits_frame`` applies it to the reduced columns of one
  frame's spectra and ``soft_checker.soft_bits`` to the others.
* ``decode_header_soft`` / ``decode_frame_soft`` - lora_decode_frame_soft_batch: block 0 at PPM
  sf - 2, the remaining blocks as ``soft_checker.decode_chain_soft`` treats a chain (whitening
  from bit offset sf - 7), every codeword by maximum likelihood with the metric's fp32 additions
  one bit at a time, in bit order.

``receive_frames_soft_host`` is ``frame_checker.receive_frames_host`` with the two decodes
swapped and the oracle's windows for the LLRs.  Comparisons against the GPU are on bit patterns
(LLRs) and integers (everything decoded)."""
from __future__ import annotations

import functools

import numpy as np

from lora_phy_amd import codes
from tests import detect_checker as dc
from tests import frame_checker as fc
from tests import soft_checker as sc

F32 = np.float32
OK, HEADER, SHORT, CRC = fc.OK, fc.HEADER, fc.SHORT, fc.CRC
MAX_FLIPS = 5


def reduced_value(k, sf: int) -> np.ndarray:
    """v'(k): grayToBinary16 of bin k rounded to the nearest multiple of four bins."""
    k = np.asarray(k, np.int64)
    return codes.gray_to_binary16((((k + 2) >> 2) & ((1 << (sf - 2)) - 1)).astype(np.uint16)).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _reduced_masks(N: int, sf: int):
    """Per bit c < sf - 2: the bins k with bit c of v'(k) set."""
    v = reduced_value(np.arange(N), sf)
    return tuple(((v >> c) & 1) == 1 for c in range(sf - 2))


def soft_bits_reduced(X: np.ndarray, sf: int) -> np.ndarray:
    """[sf] float32 LLRs of one N = 2^sf point spectrum read as a header symbol: bits 0 .. sf-3
    of v'(k), then two +0.0."""
    q = sc.spectrum_q(X)
    out = np.zeros(sf, F32)
    with np.errstate(all="ignore"):
        for c, one in enumerate(_reduced_masks(len(q), sf)):
            m1, m0 = F32(q[one].max()), F32(q[~one].max())
            out[c] = F32(0) if m1 == m0 else F32(m1 - m0)
    return out


def soft_bits_frame(spectra, sf: int, reduced=(0, 0)) -> np.ndarray:
    """[total, sf] LLRs of one frame's spectra, columns first .. first + count - 1 reduced."""
    first, count = reduced
    return np.stack([soft_bits_reduced(X, sf) if first <= s < first + count else sc.soft_bits(X, sf)
                     for s, X in enumerate(spectra)]) if len(spectra) else np.zeros((0, sf), F32)


def soft_bits_frames(M, x2d: np.ndarray, sf: int, osr: int = 1, mode: str = "legacy", hann: bool = False,
                     dechirp: bool = False, bw: int = 125000, cfo=None, time_offset=None, max_amp=None,
                     reduced=(0, 0)) -> np.ndarray:
    """soft_checker.soft_bits_frames with reduced columns: [F, total, sf] float32."""
    x2d = np.ascontiguousarray(x2d, np.complex64)
    F, L = x2d.shape
    total = L // ((1 << sf) * osr)
    llr = np.zeros((F, total, sf), F32)
    for f in range(F):
        w = dc.frame_windows(M, x2d[f], sf, osr, mode, hann, dechirp, bw,
                             0.0 if cfo is None else cfo[f], 0.0 if time_offset is None else time_offset[f],
                             0.0 if max_amp is None else max_amp[f])
        llr[f] = soft_bits_frame([M.fft(ws) for ws in w], sf, reduced)
    return llr


# ---- the decoder -------------------------------------------------------------------------------
def ml_decode(L: np.ndarray, rdd: int):
    """Maximum likelihood over the 16 codewords of rate 4 / (4 + rdd) for [n, 4 + rdd] LLRs ->
    (nibble [n], chosen codeword [n], hard word [n]): soft_checker.decode_chain_soft's rule."""
    nb = 4 + rdd
    L = np.asarray(L, F32).reshape(-1, nb)
    cw = codes.nibble_encode(np.arange(16), rdd).astype(np.int64)
    ebit = ((cw[:, None] >> np.arange(nb)[None, :]) & 1) == 1
    with np.errstate(all="ignore"):
        m = np.zeros((len(L), 16), F32)                                   # +0.0f
        for b in range(nb):                                               # in bit order
            m = (m + np.where(ebit[None, :, b], L[:, b, None], -L[:, b, None]).astype(F32)).astype(F32)
        best = np.full(len(L), -np.inf, F32)
        nib = np.zeros(len(L), np.int64)
        for x in range(16):                                               # strict '>', upward
            up = m[:, x] > best
            best = np.where(up, m[:, x], best)
            nib = np.where(up, x, nib)
        hard = ((L > 0).astype(np.int64) << np.arange(nb)[None, :]).sum(axis=1)
    return nib, cw[nib], hard


def block0_llrs(llr: np.ndarray, sf: int) -> np.ndarray:
    """The [sf - 2, 8] codeword LLRs of block 0 from the first eight rows: diagonalDeterleaveSx's
    map at PPM sf - 2, then the whitening's sign flips on codewords 5 onward."""
    ppm = sf - 2
    llr = np.asarray(llr, F32)
    L0 = np.zeros((ppm, 8), F32)
    bit, c = np.meshgrid(np.arange(8), np.arange(ppm), indexing="ij")
    L0[(c + bit) % ppm, bit] = llr[bit, c]
    w = np.frombuffer(codes.sx1272_whitening_lfsr(bytes(ppm - 5), 0, 4), np.uint8)
    flip = np.zeros((ppm, 8), bool)
    flip[5:] = ((w[:, None] >> np.arange(8)[None, :]) & 1) == 1
    return np.where(flip, -L0, L0).astype(F32)


def rest_llrs(llr: np.ndarray, sf: int, rdd: int) -> np.ndarray:
    """[S, sf] LLRs of the remaining blocks -> [blocks * sf, 4 + rdd]: soft_checker.chain_llrs
    with the whitening started at bit offset sf - 7."""
    llr = np.asarray(llr, F32)
    nb = 4 + rdd
    nblk = llr.shape[0] // nb
    L = np.zeros((nblk * sf, nb), F32)
    blk, bit, c = np.meshgrid(np.arange(nblk), np.arange(nb), np.arange(sf), indexing="ij")
    L[blk * sf + (c + bit) % sf, bit] = llr[blk * nb + bit, c]
    w = np.frombuffer(codes.sx1272_whitening_lfsr(bytes(nblk * sf), sf - 7, rdd), np.uint8)
    flip = ((w[:, None] >> np.arange(nb)[None, :]) & 1) == 1
    return np.where(flip, -L, L).astype(F32)


def _none():
    return {"status": SHORT, "nbytes": 0, "rdd": 0, "crc": 0, "nsym": 0, "errors": 0, "hdr_flips": 0}


def decode_header_soft(llr: np.ndarray, sf: int, avail=None, max_flips: int = MAX_FLIPS) -> dict:
    """Header-only mode on [S, sf] LLRs whose first eight rows are reduced columns: status (OK,
    HEADER, or SHORT for avail < 8), nbytes, rdd, crc, nsym, errors (header codewords whose
    chosen codeword differs from the hard word) and hdr_flips (bit positions in which they do)."""
    llr = np.asarray(llr, F32)
    avail = len(llr) if avail is None else min(max(int(avail), 0), len(llr))
    if avail < 8:
        return _none()
    nib, cw, hard = ml_decode(block0_llrs(llr, sf)[:5], 4)
    nib = [int(x) for x in nib]
    flips = int(sum(bin(int(a) ^ int(b)).count("1") for a, b in zip(cw, hard)))
    h0, h1, h2 = (nib[0] << 4) | nib[1], nib[2], (nib[3] << 4) | nib[4]
    if nib[3] > 1 or codes.header_checksum([h0, h1]) != h2 or (h1 >> 1) > 4 or flips > max_flips:
        return dict(_none(), status=HEADER, hdr_flips=flips)
    rdd, crc = h1 >> 1, h1 & 1
    return {"status": OK, "nbytes": h0, "rdd": rdd, "crc": crc, "nsym": fc.frame_symbols(sf, h0, rdd, crc),
            "errors": int((cw != hard).sum()), "hdr_flips": flips}


def decode_frame_soft(llr: np.ndarray, sf: int, avail=None, max_bytes: int = fc.MAX_PAYLOAD,
                      max_flips: int = MAX_FLIPS) -> dict:
    """Full decode: decode_header_soft's fields plus payload, uint8 [max_bytes]; SHORT, CRC and
    OK as frame_checker.decode_frame's."""
    llr = np.asarray(llr, F32)
    avail = len(llr) if avail is None else min(max(int(avail), 0), len(llr))
    res = decode_header_soft(llr, sf, avail, max_flips)
    res["payload"] = np.zeros(max_bytes, np.uint8)
    if res["status"] != OK:
        return res
    n, rdd, crc, nsym = res["nbytes"], res["rdd"], res["crc"], res["nsym"]
    if nsym > avail or n > max_bytes:
        res["status"] = SHORT
        return res
    nib0, cw0, hard0 = ml_decode(block0_llrs(llr, sf)[5:], 4)
    nib1, cw1, hard1 = ml_decode(rest_llrs(llr[8:nsym], sf, rdd), rdd)
    nd = 2 * (n + 2 * crc)
    nib = np.concatenate([nib0, nib1]).astype(np.int64)[:nd]
    diff = np.concatenate([cw0 != hard0, cw1 != hard1])[:nd]
    data = ((nib[0::2] << 4) | nib[1::2]).astype(np.uint8)
    res["payload"][:n] = data[:n]
    res["errors"] += int(diff.sum())
    if crc:
        c = codes.sx1272_data_checksum(data[:n].tobytes())
        if (int(data[n]) | (int(data[n + 1]) << 8)) != c:
            res["status"] = CRC
    return res


FIELDS = fc.FIELDS + ("hdr_flips",)


def decode_batch(llr3, sf: int, avail=None, max_bytes=None, max_flips: int = MAX_FLIPS) -> dict:
    """decode_frame_soft (or, with max_bytes None, decode_header_soft) per row of [F, S, sf] LLRs,
    avail None or [F] -> arrays by field."""
    rows = []
    for f, a in enumerate(np.asarray(llr3, F32)):
        av = None if avail is None else int(avail[f])
        rows.append(decode_header_soft(a, sf, av, max_flips) if max_bytes is None
                    else decode_frame_soft(a, sf, av, max_bytes, max_flips))
    out = {k: np.array([r[k] for r in rows], np.int32) for k in FIELDS}
    if max_bytes is not None:
        out["payload"] = np.stack([r["payload"] for r in rows]) if rows else np.zeros((0, max_bytes), np.uint8)
    return out


# ---- LLRs for the tests ------------------------------------------------------------------------
def frame_llrs(symbols, sf: int, rng=None, lo: float = 0.5, hi: float = 1.5) -> np.ndarray:
    """[S, sf] LLRs of a frame's data symbols (frame_checker.encode_frame's): the sign is the bit
    - of the sf - 2 bit value in the header's eight rows, whose last two entries are +0.0 - and
    the magnitude 1, or seeded uniform in lo .. hi."""
    symbols = np.asarray(symbols, np.int64)
    S = len(symbols)
    v = codes.gray_to_binary16(symbols.astype(np.uint16)).astype(np.int64)
    v[:8] = codes.gray_to_binary16((symbols[:8] >> 2).astype(np.uint16)).astype(np.int64)
    mag = np.ones((S, sf), F32) if rng is None else rng.uniform(lo, hi, (S, sf)).astype(F32)
    llr = np.where(((v[:, None] >> np.arange(sf)[None, :]) & 1) == 1, mag, -mag).astype(F32)
    llr[:8, sf - 2:] = F32(0)
    return llr


def header_cell(sf: int, j: int, bit: int):
    """(row, column) of bit `bit` of block 0's codeword j in a frame's LLRs."""
    return bit, (j - bit) % (sf - 2)


# ---- the chain ---------------------------------------------------------------------------------
def receive_frames_soft_host(O, x, sf: int, osr: int, max_symbols: int, hop: int, sync: int = 0x12,
                             thresh_db: float = 0.0, first: int = 0, cand_capacity=None,
                             max_bytes: int = fc.MAX_PAYLOAD, max_flips: int = MAX_FLIPS):
    """stream.receive_frames_device(soft=True) on one row, on the CPU:
    frame_checker.receive_frames_host with decode_header_soft and decode_frame_soft on the LLRs of
    the oracle's windows (columns 2 - 9 reduced), each slot rebuilt with the cfo, time offset and
    maximum amplitude of the oracle's own demodulation of it."""
    from tests import scan_checker as scn

    x = np.ascontiguousarray(x, np.complex64)
    step = (1 << sf) * osr
    L = len(x)
    m = scn.scan_host(O, x, sf, osr, hop, False, True)
    cands = fc.find_candidates_host(m, hop, sf, osr, sync, thresh_db, L)
    cap = -(-L // (4 * step)) if cand_capacity is None else cand_capacity
    kept = cands[:cap]

    def llrs(rows):
        syms, sy, cfo, toff, cnt = O.demod_frames(rows, sf, osr, False, True)
        amp = np.array([max_amplitude(O, r, sf, osr) for r in rows], F32)
        return soft_bits_frames(O, rows, sf, osr, "legacy", False, True, 125000, cfo, toff, amp, (2, 8)), \
            (syms, sy, cfo, toff, cnt)

    status, hsym = np.zeros(len(kept), np.int32), np.zeros(len(kept), np.int32)
    if len(kept):
        heads = fc.gather_host(x, kept, [10 * step] * len(kept), 10 * step)
        llr, _ = llrs(heads)
        for j in range(len(kept)):
            h = decode_header_soft(llr[j, 2:], sf, None, max_flips)
            status[j], hsym[j] = h["status"], h["nsym"]
    starts, nsym, end = fc.select_frames_host(kept, status, hsym, step, L, max_symbols, first)
    out = {"candidates": cands, "starts": starts, "nsym": nsym, "end": end, "frames": []}
    if len(starts):
        cut = (2 + max_symbols) * step
        frames = fc.gather_host(x, starts, (2 + nsym.astype(np.int64)) * step, cut)
        llr, (syms, sy, cfo, toff, cnt) = llrs(frames)
        for j in range(len(starts)):
            f = decode_frame_soft(llr[j, 2:], sf, int(nsym[j]), max_bytes, max_flips)
            f.update(symbols=syms[j, :cnt[j]].copy(), sync=sy[j], cfo=cfo[j], time_offset=toff[j], padded=frames[j],
                     llr=llr[j])
            out["frames"].append(f)
    return out


def max_amplitude(M, x: np.ndarray, sf: int, osr: int = 1) -> np.float32:
    """The frame maximum the legacy demodulator normalises by (LoRaDemod.cpp:59-67) on a
    dechirping plan: the largest |re| or |im| of the dechirped frame."""
    x = np.ascontiguousarray(x, np.complex64)
    if len(x) == 0:
        return F32(0)
    y = M.dechirp(x, sf, osr)
    return F32(max(np.abs(y.real).max(), np.abs(y.imag).max()))
