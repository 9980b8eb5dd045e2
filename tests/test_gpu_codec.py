"""GPU: the payload codec (lora_phy_amd.codec over csrc/lora_codec.hip) against the host
implementation lora_phy_amd.codes, which tests/test_codes.py pins to the compiled reference.
Everything is integer work: every comparison is exact."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from lora_phy_amd import codes  # noqa: E402

# Lanes per frame of k_codec_decode by bytes per frame n = S // 2: 1, 2, 4, 8, 16, 32 lanes
# up to n = 32, 64 lanes (striding the frame) up to n = 256, a whole workgroup beyond.  The
# symbol counts on both sides of every step:
DECODE_THRESHOLDS = [3, 4, 5, 6, 9, 10, 17, 18, 33, 34, 65, 66, 513, 514]
DECODE_S = sorted(set([0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 510] + DECODE_THRESHOLDS))
DECODE_F = (1, 63, 65, 257)
POOL = 37  # distinct frames per symbol count (31 counts x 37 = 1,147 <= 4,096 host-checked frames)
SENT8, SENT32 = 0xA5, 0x7F7F7F7F


@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import lora_phy_amd

    return lora_phy_amd


def dev_u16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint16)).cuda()


def dev_u8(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).cuda()


def with_crc(payload: bytes) -> bytes:
    """The host construction of tests/test_codes.py::test_decode_with_crc_and_batches."""
    crc = codes.sx1272_data_checksum(payload[2:])
    return payload + bytes([crc & 0xFF, crc >> 8])


def host_counts(sym):
    lo = np.asarray(sym, np.int64)[..., : (np.shape(sym)[-1] // 2) * 2] & 0xFF
    return codes.DEC_H84_ERR[lo].sum(-1), codes.DEC_H84_BAD[lo].sum(-1)


# ---------------------------------------------------------------------------------
# Decode: every codeword
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [65536, 256])
def test_decode_every_codeword(amd, count):
    """Every uint16 value as a symbol (one multi-wave frame: only the low byte counts), and
    the 256 byte values."""
    sym = np.arange(count, dtype=np.uint16)
    res = amd.codec.decode(dev_u16(sym))
    want, ok = codes.decode_with_crc(sym)
    err, bad = host_counts(sym)
    assert np.array_equal(res.payload.cpu().numpy(), want)
    assert bool(res.crc_ok.cpu()[0]) == ok
    assert int(res.errors.cpu()[0]) == err and int(res.bad.cpu()[0]) == bad


def test_decode_corrects_every_single_bit_flip(amd):
    nib = np.repeat(np.arange(16), 8)
    sym = codes.ENC_H84[nib].astype(np.uint16) ^ (1 << np.tile(np.arange(8), 16)).astype(np.uint16)
    res = amd.codec.decode(dev_u16(sym))
    got = res.payload.cpu().numpy()
    assert np.array_equal(np.stack([got >> 4, got & 0xF], -1).reshape(-1), nib)
    assert int(res.errors.cpu()[0]) == 128 and int(res.bad.cpu()[0]) == 0


# ---------------------------------------------------------------------------------
# Decode: frame shapes
# ---------------------------------------------------------------------------------
def frame_pool(S, rng):
    """POOL distinct frames of S symbols: random uint16 symbols, frames built with a CRC
    (garbage in the symbols' high byte and in an odd trailing symbol), and frames built
    with a CRC and one payload bit flipped afterwards.  -> symbols, kind (0, 1, 2)."""
    n = S // 2
    sym = rng.integers(0, 1 << 16, (POOL, S)).astype(np.uint16)
    kind = np.zeros(POOL, int)
    if n >= 4:
        for i in range(1, POOL, 2):
            frame = bytearray(with_crc(rng.integers(0, 256, n - 2).astype(np.uint8).tobytes()))
            kind[i] = 1
            if i % 3 == 0:  # flipped after the CRC was made: a covered byte, or the CRC itself
                j = int(rng.integers(2, n - 2)) if n > 4 else n - 1
                frame[j] ^= 1 << int(rng.integers(0, 8))
                kind[i] = 2
            sym[i, :2 * n] = codes.lora_encode(bytes(frame)) | (sym[i, :2 * n] & 0xFF00)
    return sym, kind


@pytest.fixture(scope="module")
def decode_reference():
    """Host results per symbol count, computed once: payload, crc_ok, errors, bad of the pool."""
    rng = np.random.default_rng(7)
    ref = {}
    for S in DECODE_S:
        sym, kind = frame_pool(S, rng)
        pay = np.zeros((POOL, S // 2), np.uint8)
        ok = np.zeros(POOL, bool)
        for i in range(POOL):
            pay[i], ok[i] = codes.decode_with_crc(sym[i])
        err, bad = host_counts(sym)
        ref[S] = (sym, kind, pay, ok, err, bad)
    return ref


@pytest.mark.parametrize("S", DECODE_S)
def test_decode_frame_shapes(amd, decode_reference, S):
    """Every frame of every batch equals codes.decode_with_crc's result for it (frame f is
    pool frame f mod 37, so the host CRC runs on 37 frames per symbol count); rows are S + 5
    symbols apart, the outputs sit inside sentinels and start as garbage."""
    sym, kind, pay, ok, err, bad = decode_reference[S]
    n = S // 2
    if S < 8:
        assert not ok.any()
    if S == 8:  # the checksum over zero bytes
        provided = pay[:, 2].astype(int) | (pay[:, 3].astype(int) << 8)
        assert np.array_equal(ok, provided == codes.sx1272_data_checksum(b""))
    if n >= 4:
        assert ok[kind == 1].all() and not ok[kind == 2].any()
    for F in DECODE_F:
        idx = np.arange(F) % POOL
        buf = np.random.default_rng(F).integers(0, 1 << 16, (F, S + 5)).astype(np.uint16)
        buf[:, :S] = sym[idx]
        d_sym = dev_u16(buf)[:, :S]
        d_pay = torch.full((F, n + 6), SENT8, dtype=torch.uint8, device="cuda")
        d_ok = torch.ones(F + 2, dtype=torch.bool, device="cuda")
        d_err = torch.full((F + 2,), SENT32, dtype=torch.int32, device="cuda")
        d_bad = torch.full((F + 2,), SENT32, dtype=torch.int32, device="cuda")
        out = amd.codec.DecodeResult(payload=d_pay[:, 3:3 + n], crc_ok=d_ok[1:F + 1], errors=d_err[1:F + 1],
                                     bad=d_bad[1:F + 1])
        res = amd.codec.decode(d_sym, out=out)
        assert res is out
        torch.cuda.synchronize()
        h_pay = d_pay.cpu().numpy()
        assert np.array_equal(h_pay[:, 3:3 + n], pay[idx]), (S, F)
        assert (h_pay[:, :3] == SENT8).all() and (h_pay[:, 3 + n:] == SENT8).all(), (S, F)
        assert np.array_equal(d_ok.cpu().numpy(), np.concatenate([[True], ok[idx], [True]])), (S, F)
        assert np.array_equal(d_err.cpu().numpy(), np.concatenate([[SENT32], err[idx], [SENT32]])), (S, F)
        assert np.array_equal(d_bad.cpu().numpy(), np.concatenate([[SENT32], bad[idx], [SENT32]])), (S, F)


def test_decode_single_frame_is_one_dimensional(amd):
    frame = with_crc(bytes(range(20)))
    res = amd.codec.decode(dev_u16(codes.lora_encode(frame)))
    assert res.payload.shape == (22,) and bytes(res.payload.cpu().numpy()) == frame
    assert res.crc_ok.shape == (1,) and bool(res.crc_ok.cpu()[0])


# ---------------------------------------------------------------------------------
# Encode
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("nbytes", [0, 1, 2, 31, 32, 33, 255])
def test_encode_equals_host(amd, nbytes):
    F = 5
    pay = np.random.default_rng(nbytes).integers(0, 256, (F, nbytes)).astype(np.uint8)
    d_pay = dev_u8(pay)
    plain = amd.codec.encode(d_pay).cpu().numpy()
    framed = amd.codec.encode(d_pay, append_crc=True)
    assert plain.shape == (F, 2 * nbytes) and framed.shape == (F, 2 * nbytes + 4)
    h_framed = framed.cpu().numpy()
    for f in range(F):
        assert np.array_equal(plain[f], codes.lora_encode(pay[f].tobytes())), f
        assert np.array_equal(h_framed[f], codes.lora_encode(with_crc(pay[f].tobytes()))), f
    # the round trip returns the payload and its checksum; the check needs 4 bytes
    res = amd.codec.decode(framed)
    got = res.payload.cpu().numpy()
    for f in range(F):
        assert bytes(got[f]) == with_crc(pay[f].tobytes())
    assert (res.crc_ok.cpu().numpy() == (nbytes >= 2)).all()
    assert not res.errors.cpu().numpy().any() and not res.bad.cpu().numpy().any()


def test_encode_into_strided_rows(amd):
    pay = np.random.default_rng(3).integers(0, 256, (9, 20)).astype(np.uint8)
    d_pay = dev_u8(np.pad(pay, ((0, 0), (0, 3))))[:, :20]
    d_sym = torch.full((9, 51), 0xBEEF, dtype=torch.int32, device="cuda").to(torch.uint16)
    out = amd.codec.encode(d_pay, append_crc=True, out=d_sym[:, :44])
    assert out.data_ptr() == d_sym.data_ptr()
    h = d_sym.cpu().numpy()
    assert (h[:, 44:] == 0xBEEF).all()
    for f in range(9):
        assert np.array_equal(h[f, :44], codes.lora_encode(with_crc(pay[f].tobytes())))


# ---------------------------------------------------------------------------------
# The coding chain
# ---------------------------------------------------------------------------------
def chain_sizes(sf):
    # one byte; exactly one block (2 n <= sf, as many as fit); two blocks (the first size that
    # needs a second, and the one that fills it); 64; 255
    return sorted({1, sf // 2, sf // 2 + 1, sf, 64, 255})


@pytest.mark.parametrize("rdd", range(5))
@pytest.mark.parametrize("sf", range(6, 13))
def test_chain_equals_host(amd, sf, rdd):
    rng = np.random.default_rng(100 * sf + rdd)
    F = 8
    for n in chain_sizes(sf):
        pay = rng.integers(0, 256, (F, n)).astype(np.uint8)
        want = np.stack([codes.encode_chain(pay[f].tobytes(), sf, rdd)["symbols"] for f in range(F)])
        got = amd.codec.encode_chain(dev_u8(pay), sf, rdd)
        assert got.shape == want.shape == (F, amd.codec.chain_symbols(sf, rdd, n))
        assert np.array_equal(got.cpu().numpy(), want), (sf, rdd, n)
        back = amd.codec.decode_chain(got, sf, rdd, n)
        assert np.array_equal(back.payload.cpu().numpy(), pay) and not back.errors.cpu().numpy().any()
        # random uint16 symbols (bits above sf set: the host chain defines the result), three
        # trailing symbols past the last whole block, and a truncating nbytes
        S = want.shape[1] + 3
        sym = rng.integers(0, 1 << 16, (F, S)).astype(np.uint16)
        d_sym = dev_u16(sym)
        for nb in sorted({n, (n + 1) // 2}):
            res = amd.codec.decode_chain(d_sym, sf, rdd, nb)
            h_pay, h_err = res.payload.cpu().numpy(), res.errors.cpu().numpy()
            for f in range(F):
                ref = codes.decode_chain(sym[f], sf, rdd, nb)
                assert np.array_equal(h_pay[f], ref["payload"]), (sf, rdd, n, nb, f)
                assert h_err[f] == int(ref["errors"][:2 * nb].sum()), (sf, rdd, n, nb, f)
        # without its last symbol the frame has lost a block: the same nbytes no longer fits
        with pytest.raises(amd.LoraError):
            amd.codec.decode_chain(got[:, :-1], sf, rdd, n)


@pytest.mark.parametrize("rdd", [1, 2, 3, 4])
@pytest.mark.parametrize("sf", [7, 12])
def test_chain_one_flipped_bit_per_codeword(amd, sf, rdd):
    """One bit flipped in every transmitted codeword: Hamming 7/4 and 8/4 correct it, the two
    parity codes flag it.  (The flips are made on the host chain's whitened codewords, which
    are then interleaved and Gray-mapped as the host chain does.)"""
    rng = np.random.default_rng(sf + rdd)
    F, n = 4, 33
    pay = rng.integers(0, 256, (F, n)).astype(np.uint8)
    sym = []
    for f in range(F):
        wh = codes.encode_chain(pay[f].tobytes(), sf, rdd)["whitened"].copy()
        wh ^= (1 << rng.integers(0, 4 + rdd, len(wh))).astype(np.uint8)
        sym.append(codes.binary_to_gray16(codes.diagonal_interleave(wh, sf, rdd)))
    res = amd.codec.decode_chain(dev_u16(np.stack(sym)), sf, rdd, n)
    assert (res.errors.cpu().numpy() == 2 * n).all()
    if rdd >= 3:
        assert np.array_equal(res.payload.cpu().numpy(), pay)


# ---------------------------------------------------------------------------------
# End to end on the device
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("sf,F,n", [(7, 8, 14), (9, 3, 5)])
def test_end_to_end_library_chain(amd, sf, F, n):
    """bytes -> encode + CRC -> modulate -> demodulate -> decode, all on the device.  (At SF7
    the modulator carries 7 of a codeword's 8 bits: the decoder sees the top check bit of
    half the codewords flipped and corrects it - errors are flagged, none is bad.)"""
    pay = torch.randint(0, 256, (F, n), dtype=torch.uint8, device="cuda",
                        generator=torch.Generator("cuda").manual_seed(sf))
    mod, demod = amd.LoRaMod(sf), amd.LoRaDemod(sf)
    res = demod.work_payload(mod.work_payload(pay, append_crc=True))
    assert res.payload.is_cuda and res.payload.shape == (F, n + 2)
    ok = (res.payload[:, :n] == pay).all() & res.crc_ok.all() & demod.sync_ok().all() & (res.bad == 0).all()
    assert bool(ok)  # the first value to leave the device
    assert bytes(res.payload[0].cpu().numpy()) == with_crc(bytes(pay[0].cpu().numpy()))
    # nbytes: the CRC check over the first 2 * nbytes symbols only (here: too few for the CRC's place)
    short = demod.work_payload(mod.work_payload(pay, append_crc=True), nbytes=n)
    assert short.payload.shape == (F, n) and torch.equal(short.payload, pay)


def test_end_to_end_lora_chain(amd):
    sf, F, n = 7, 8, 14
    pay = torch.randint(0, 256, (F, n), dtype=torch.uint8, device="cuda",
                        generator=torch.Generator("cuda").manual_seed(1))
    mod, demod = amd.LoRaMod(sf, cr=4), amd.LoRaDemod(sf, cr=4)
    res = demod.work_payload(mod.work_payload(pay, chain="lora"), chain="lora")
    assert res.payload.shape == (F, n)
    assert bool((res.payload == pay).all() & (res.errors == 0).all() & demod.sync_ok().all())
    one = demod.work_payload(mod.work_payload(pay[0], chain="lora"), nbytes=n, chain="lora")
    assert one.payload.shape == (n,) and torch.equal(one.payload, pay[0])


# ---------------------------------------------------------------------------------
# Contract: stream, graph capture, no allocation
# ---------------------------------------------------------------------------------
def framed_batch(F, n, seed):
    rng = np.random.default_rng(seed)
    frames = [with_crc(rng.integers(0, 256, n).astype(np.uint8).tobytes()) for _ in range(F)]
    return np.stack([np.frombuffer(fr, np.uint8) for fr in frames]), np.stack([codes.lora_encode(fr) for fr in frames])


def test_decode_runs_on_the_callers_stream(amd):
    """The symbols are produced on a side stream behind a long-running kernel; a decode on any
    other stream would read the buffer before they are there."""
    pay, sym = framed_batch(300, 30, 5)
    src = dev_u16(sym)
    d_sym = torch.zeros_like(src)
    big = torch.randn(4096, 4096, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(4):
            big = big @ big * 1e-3
        d_sym.copy_(src)
        res = amd.codec.decode(d_sym)
    s.synchronize()
    assert np.array_equal(res.payload.cpu().numpy(), pay) and res.crc_ok.cpu().numpy().all()


def test_decode_graph_capture_and_replay(amd):
    pay, sym = framed_batch(500, 30, 6)
    d_sym = dev_u16(sym)
    out = amd.codec.decode(d_sym)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        amd.codec.decode(d_sym, out=out)
    torch.cuda.current_stream().wait_stream(s)
    out.payload.zero_()
    out.crc_ok.zero_()
    with torch.cuda.graph(g):
        amd.codec.decode(d_sym, out=out)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.payload.cpu().numpy(), pay) and out.crc_ok.cpu().numpy().all()
    pay2, sym2 = framed_batch(500, 30, 8)  # new input in the same buffer
    d_sym.copy_(dev_u16(sym2))
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.payload.cpu().numpy(), pay2) and out.crc_ok.cpu().numpy().all()


def test_no_device_allocation_per_call(amd):
    pay, sym = framed_batch(64, 20, 9)
    d_sym, d_pay = dev_u16(sym), dev_u8(pay)
    out = amd.codec.decode(d_sym)
    enc = amd.codec.encode(d_pay[:, :20], append_crc=True)
    ch = amd.codec.encode_chain(d_pay, 8, 4)
    back = amd.codec.decode_chain(ch, 8, 4, 22)
    torch.cuda.synchronize()
    stats = torch.cuda.memory_stats()["allocation.all.allocated"]
    before = torch.cuda.memory_allocated()
    for _ in range(3):
        amd.codec.decode(d_sym, out=out)
        amd.codec.encode(d_pay[:, :20], append_crc=True, out=enc)
        amd.codec.encode_chain(d_pay, 8, 4, out=ch)
        amd.codec.decode_chain(ch, 8, 4, 22, out=back)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == stats
    assert np.array_equal(out.payload.cpu().numpy(), pay) and np.array_equal(back.payload.cpu().numpy(), pay)
    assert torch.equal(enc, d_sym)


def test_wrappers_reject_bad_tensors(amd):
    sym = torch.zeros((4, 16), dtype=torch.int32, device="cuda").to(torch.uint16)
    pay = torch.zeros((4, 8), dtype=torch.uint8, device="cuda")
    with pytest.raises(TypeError):
        amd.codec.decode(sym.cpu())
    with pytest.raises(TypeError):
        amd.codec.decode(sym.to(torch.float32))
    with pytest.raises(TypeError):
        amd.codec.encode(pay.to(torch.int32))
    with pytest.raises(ValueError):
        amd.codec.decode(torch.zeros((16, 4), dtype=torch.int32, device="cuda").to(torch.uint16).t())
    with pytest.raises(ValueError):
        amd.codec.encode(pay, out=torch.zeros((4, 15), dtype=torch.int32, device="cuda").to(torch.uint16))
    with pytest.raises(ValueError):
        amd.codec.encode(torch.zeros((1, 256), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        amd.codec.decode_chain(sym, 7, 5, 4)
    with pytest.raises(amd.LoraError):
        amd.codec.decode_chain(sym, 7, 4, 8)  # 16 symbols are two blocks: 14 codewords, 7 bytes
