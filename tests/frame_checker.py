"""The self-describing frame (include/lora_mi355x.h, "Self-describing frames") restated in numpy
on top of lora_phy_amd.codes, whose primitives tests/test_codes.py pins to the reference.  It is
the checker of lora_encode_frame_batch / lora_decode_frame_batch (tests/test_gpu_frame.py) and
is itself checked by tests/test_frame_checker.py.

The frame: an explicit header (payload bytes n, coding rate rdd, CRC flag, 5-bit checksum) as
five Hamming 8/4 codewords in a first block of sf - 2 codewords at rate 4/8 whose eight symbols
carry sf - 2 bits each (<< 2: a +-1 bin error does not reach them); the block's other sf - 7
codewords are the first data nibbles.  The remaining data nibbles follow in blocks of sf
codewords at rate 4 / (4 + rdd), as the coding chain's.  Data = payload, then with the CRC flag
the SX1272 data checksum of the whole payload, low byte first."""
import numpy as np

from lora_phy_amd import codes

OK, HEADER, SHORT, CRC = 0, 1, 2, 3
MAX_PAYLOAD = 255


def frame_symbols(sf: int, n: int, rdd: int, crc: int) -> int:
    nd = 2 * (n + 2 * crc)
    k = max(nd - (sf - 7), 0)
    return 8 + -(-k // sf) * (4 + rdd)


def header_nibbles(n: int, rdd: int, crc: int):
    h0, h1 = n, (rdd << 1) | crc
    h2 = codes.header_checksum([h0, h1])
    return [h0 >> 4, h0 & 15, h1 & 15, h2 >> 4, h2 & 15]


def data_bytes(payload: bytes, crc: int) -> bytes:
    payload = bytes(payload)
    if not crc:
        return payload
    c = codes.sx1272_data_checksum(payload)
    return payload + bytes([c & 0xFF, c >> 8])


def encode_frame(payload: bytes, sf: int, rdd: int, crc: int) -> np.ndarray:
    """-> the frame's data symbols, uint16 [frame_symbols(sf, len(payload), rdd, crc)]."""
    assert 7 <= sf <= 12 and 0 <= rdd <= 4 and crc in (0, 1) and len(payload) <= MAX_PAYLOAD
    nib = codes.payload_nibbles(data_bytes(payload, crc))
    nh = sf - 7
    # block 0: five header codewords, then sf - 7 whitened data codewords (zero ones when the
    # data has run out)
    cw0 = np.zeros(sf - 2, np.uint8)
    cw0[:5] = codes.encode_hamming84(header_nibbles(len(payload), rdd, crc))
    first = nib[:nh]
    cw0[5:5 + len(first)] = codes.encode_hamming84(first)
    cw0[5:] = np.frombuffer(codes.sx1272_whitening_lfsr(cw0[5:].tobytes(), 0, 4), np.uint8)
    sym0 = codes.binary_to_gray16(codes.diagonal_interleave(cw0, sf - 2, 4)).astype(np.uint16) << 2
    # the remaining blocks
    rest = nib[nh:]
    ncw = -(-len(rest) // sf) * sf
    cw = np.zeros(ncw, np.uint8)
    cw[:len(rest)] = codes.nibble_encode(rest, rdd)
    wh = np.frombuffer(codes.sx1272_whitening_lfsr(cw.tobytes(), nh, rdd), np.uint8)
    sym = codes.binary_to_gray16(codes.diagonal_interleave(wh, sf, rdd))
    out = np.concatenate([sym0, sym]).astype(np.uint16)
    assert len(out) == frame_symbols(sf, len(payload), rdd, crc)
    return out


def _block0(symbols, sf: int) -> np.ndarray:
    """The sf - 2 codewords of the first block from its eight symbols."""
    s = np.asarray(symbols[:8]).astype(np.int64) & 0xFFFF
    r = ((s + 2) >> 2) & ((1 << (sf - 2)) - 1)
    return codes.diagonal_deinterleave(codes.gray_to_binary16(r), sf - 2, 4)


def decode_header(symbols, sf: int, avail=None) -> dict:
    """Header-only mode: status (OK, HEADER, or SHORT for avail < 8), nbytes, rdd, crc, nsym and
    errors (header codewords that flagged an error)."""
    avail = len(symbols) if avail is None else min(max(int(avail), 0), len(symbols))
    none = {"status": SHORT, "nbytes": 0, "rdd": 0, "crc": 0, "nsym": 0, "errors": 0}
    if avail < 8:
        return none
    nib, err, bad = codes.decode_hamming84(_block0(symbols, sf)[:5])
    nib = [int(x) for x in nib]
    h0, h1, h2 = (nib[0] << 4) | nib[1], nib[2], (nib[3] << 4) | nib[4]
    if bad.any() or nib[3] > 1 or codes.header_checksum([h0, h1]) != h2 or (h1 >> 1) > 4:
        return dict(none, status=HEADER)
    rdd, crc = h1 >> 1, h1 & 1
    return {"status": OK, "nbytes": h0, "rdd": rdd, "crc": crc, "nsym": frame_symbols(sf, h0, rdd, crc),
            "errors": int((err | bad).sum())}


def decode_frame(symbols, sf: int, avail=None, max_bytes: int = MAX_PAYLOAD) -> dict:
    """Full decode: decode_header's fields plus payload, uint8 [max_bytes] (zeros beyond nbytes).
    A frame of more symbols than avail, or of more bytes than max_bytes, is SHORT with its fields
    set, a zero payload and the header's errors."""
    symbols = np.asarray(symbols)
    avail = len(symbols) if avail is None else min(max(int(avail), 0), len(symbols))
    res = decode_header(symbols, sf, avail)
    res["payload"] = np.zeros(max_bytes, np.uint8)
    if res["status"] != OK:
        return res
    n, rdd, crc, nsym = res["nbytes"], res["rdd"], res["crc"], res["nsym"]
    if nsym > avail or n > max_bytes:
        res["status"] = SHORT
        return res
    nh = sf - 7
    cw0 = _block0(symbols, sf)[5:]
    cw0 = np.frombuffer(codes.sx1272_whitening_lfsr(cw0.tobytes(), 0, 4), np.uint8)
    nib0, err0, bad0 = codes.decode_hamming84(cw0)
    di = codes.diagonal_deinterleave(codes.gray_to_binary16(symbols[8:nsym]), sf, rdd)
    dw = np.frombuffer(codes.sx1272_whitening_lfsr(di.tobytes(), nh, rdd), np.uint8)
    nib1, err1 = codes.nibble_decode(dw, rdd)
    nd = 2 * (n + 2 * crc)
    nib = np.concatenate([nib0 & 0xF, nib1]).astype(np.int64)[:nd]
    err = np.concatenate([err0 | bad0, err1])[:nd]
    data = ((nib[0::2] << 4) | nib[1::2]).astype(np.uint8)
    res["payload"][:n] = data[:n]
    res["errors"] += int(err.sum())
    if crc:
        c = codes.sx1272_data_checksum(data[:n].tobytes())
        if (int(data[n]) | (int(data[n + 1]) << 8)) != c:
            res["status"] = CRC
    return res


FIELDS = ("status", "nbytes", "rdd", "crc", "nsym", "errors")


def decode_batch(symbols, sf: int, avail=None, max_bytes=None) -> dict:
    """decode_frame (or, with max_bytes None, decode_header) per row of [F, S] symbols, avail
    None or [F] -> arrays by field."""
    rows = []
    for f, s in enumerate(np.asarray(symbols)):
        a = None if avail is None else int(avail[f])
        rows.append(decode_header(s, sf, a) if max_bytes is None else decode_frame(s, sf, a, max_bytes))
    out = {k: np.array([r[k] for r in rows], np.int32) for k in FIELDS}
    if max_bytes is not None:
        out["payload"] = np.stack([r["payload"] for r in rows]) if rows else np.zeros((0, max_bytes), np.uint8)
    return out


def encode_batch(payload, nbytes, sf: int, rdd: int, crc: int):
    """encode_frame per row of [F, max_bytes] payload with nbytes [F] -> symbols [F, S] (zeros
    beyond each frame's nsym, S the symbols of a max_bytes frame) and nsym [F]."""
    payload = np.asarray(payload, np.uint8)
    S = frame_symbols(sf, payload.shape[1], rdd, crc)
    sym = np.zeros((payload.shape[0], S), np.uint16)
    nsym = np.zeros(payload.shape[0], np.int32)
    for f in range(payload.shape[0]):
        s = encode_frame(payload[f, :int(nbytes[f])].tobytes(), sf, rdd, crc)
        sym[f, :len(s)] = s
        nsym[f] = len(s)
    return sym, nsym


def gather_host(flat, at, length, cut: int) -> np.ndarray:
    """lora_gather_frames_batch: out[s, t] = flat[at[s] + t] for t < length[s], 0 up to cut; a
    slot whose at is negative or beyond the stream is zeros, length is clamped to 0..cut and to
    the stream's end."""
    flat = np.asarray(flat)
    out = np.zeros((len(at), cut), flat.dtype)
    for s, (a, n) in enumerate(zip(at, length)):
        a, n = int(a), int(n)
        if 0 <= a < len(flat):
            n = min(max(n, 0), cut, len(flat) - a)
            out[s, :n] = flat[a:a + n]
    return out


# ---------------------------------------------------------------------------------
# The finder of self-describing frames (lora_phy_amd/stream.py: find_candidates_device,
# select_frames_device, receive_frames_device), window by window and slot by slot
# ---------------------------------------------------------------------------------
def synthetic_scan(seed, sf, k, W, frac, sync=0x12):
    """A scan that stresses the candidate list (after tests/test_gpu_find.synthetic): chains of
    windows whose peaks differ as the sync symbols do, NaN power and -inf floors sprinkled in."""
    rng = np.random.default_rng(seed)
    N = 1 << sf
    sw0, sw1 = (sync >> 4) << (sf - 4), (sync & 15) << (sf - 4)
    index = rng.integers(0, N, W)
    for w in np.flatnonzero(rng.random(max(W - k, 0)) < frac):
        index[w + k] = (index[w] + sw1 - sw0) % N
    power = rng.normal(0, 3, W).astype(np.float32)
    power_avg = (power - rng.normal(2, 3, W).astype(np.float32)).astype(np.float32)
    power[rng.random(W) < 0.01] = np.nan
    power_avg[rng.random(W) < 0.01] = -np.inf
    return {"index": index.astype(np.uint16), "power": power, "power_avg": power_avg}


def find_candidates_host(m, hop: int, sf: int, osr: int, sync: int = 0x12, thresh_db: float = 0.0,
                         row_len=None) -> np.ndarray:
    """Every start one row's scan lists (1-D arrays, or [1, W]), int64, uncut by any capacity: the
    candidate rule and refinement of scan_checker.find_frames_host, a start listed when it lies
    in the row with ten symbols after it and differs from the last listed one."""
    N = 1 << sf
    step = N * osr
    assert 6 <= sf <= 12 and step % hop == 0 and step // hop >= 2
    k = step // hop
    sw0, sw1 = (sync >> 4) << (sf - 4), (sync & 15) << (sf - 4)
    index = np.asarray(m["index"]).reshape(-1).astype(np.int64)
    with np.errstate(invalid="ignore"):
        snr = np.asarray(m["power"], np.float32).reshape(-1) - np.asarray(m["power_avg"], np.float32).reshape(-1)
        ok = snr >= np.float32(thresh_db)  # NaN fails
    W = len(index)
    if row_len is None:
        row_len = (W - 1) * hop + step if W else 0
    starts = []
    for w in range(max(W - k, 0)):
        if not (ok[w] and ok[w + k] and (index[w + k] - index[w]) % N == (sw1 - sw0) % N):
            continue
        d = (index[w] - sw0) % N
        if d >= N // 2:
            d -= N
        start = w * hop - d * osr
        if start >= 0 and start + 10 * step <= row_len and (not starts or starts[-1] != start):
            starts.append(start)
    return np.array(starts, np.int64)


def select_frames_host(starts, status, nsym, step: int, row_len: int, max_symbols: int, first: int = 0):
    """The greedy pass over one row's slots, in slot order -> (accepted starts int64, their nsym
    int32, end), uncut by any capacity."""
    out, outn = [], []
    for s, st, n in zip(starts, status, nsym):
        s, n = int(s), int(n)
        if st == OK and 0 <= n <= max_symbols and s >= 0 and s >= first and s + (2 + n) * step <= row_len:
            out.append(s)
            outn.append(n)
            first = s + (2 + n) * step
    return np.array(out, np.int64), np.array(outn, np.int32), first


def to_slots(values, capacity: int, fill, dtype) -> np.ndarray:
    """What a row's `capacity` slots hold for the listed `values`: the first min(count, capacity)
    of them, then `fill`.  (The count beside them is len(values): it does not depend on capacity.)"""
    out = np.full(capacity, fill, dtype)
    out[:min(len(values), capacity)] = values[:capacity]
    return out


def receive_frames_host(O, x, sf: int, osr: int, max_symbols: int, hop: int, sync: int = 0x12,
                        thresh_db: float = 0.0, first: int = 0, cand_capacity=None, max_bytes: int = MAX_PAYLOAD):
    """stream.receive_frames_device on one row, on the CPU: the oracle's scan and demodulator
    (the device's equal them bit for bit), this file's candidates, header gate, pass and decode.
    -> dict: candidates (all listed starts), starts, nsym, end, and per accepted frame status,
    nbytes, rdd, crc, errors, payload and the demodulated symbols, sync, cfo, time_offset."""
    from tests import scan_checker as sc

    x = np.ascontiguousarray(x, np.complex64)
    step = (1 << sf) * osr
    L = len(x)
    m = sc.scan_host(O, x, sf, osr, hop, False, True)
    cands = find_candidates_host(m, hop, sf, osr, sync, thresh_db, L)
    cap = -(-L // (4 * step)) if cand_capacity is None else cand_capacity
    kept = cands[:cap]
    status, hsym = np.zeros(len(kept), np.int32), np.zeros(len(kept), np.int32)
    if len(kept):
        heads = gather_host(x, kept, [10 * step] * len(kept), 10 * step)
        syms, _, _, _, cnt = O.demod_frames(heads, sf, osr, False, True)
        for j in range(len(kept)):
            h = decode_header(syms[j, :cnt[j]], sf)
            status[j], hsym[j] = h["status"], h["nsym"]
    starts, nsym, end = select_frames_host(kept, status, hsym, step, L, max_symbols, first)
    out = {"candidates": cands, "starts": starts, "nsym": nsym, "end": end, "frames": []}
    if len(starts):
        cut = (2 + max_symbols) * step
        frames = gather_host(x, starts, (2 + nsym.astype(np.int64)) * step, cut)
        syms, sy, cfo, toff, cnt = O.demod_frames(frames, sf, osr, False, True)
        for j in range(len(starts)):
            f = decode_frame(syms[j, :cnt[j]], sf, int(nsym[j]), max_bytes)
            f.update(symbols=syms[j, :cnt[j]].copy(), sync=sy[j], cfo=cfo[j], time_offset=toff[j], padded=frames[j])
            out["frames"].append(f)
    return out
