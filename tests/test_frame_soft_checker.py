"""CPU: the soft path through the self-describing frame as tests/frame_soft_checker.py restates
it (include/lora_mi355x.h: lora_demod_soft_bits_frame_batch's reduced columns and
lora_decode_frame_soft_batch): the reduced column is bits 2 .. sf-1 of the rotated spectrum, clean
LLRs decode to what was planted over the whole grid of shapes, the soft header mends what the
hard one cannot and max_flips bounds how much, ties and non-finite LLRs follow the scan rule,
and on whole noisy frames the soft decoder loses at most half the frames the hard one loses
while its header gate lets no more noise through.  The kernels are held to the same checker in
tests/test_gpu_frame_soft.py."""
import numpy as np
import pytest

from lora_phy_amd import codes
from tests import detect_checker as dc
from tests import frame_checker as fc
from tests import frame_soft_checker as fs
from tests import soft_checker as sc

SFS = range(7, 13)


def sizes(sf):
    return (0, 1, 2, 3, 4, 5, sf, 16, 17, 255)


def payload_of(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n).astype(np.uint8).tobytes()


@pytest.fixture(scope="module")
def O():
    from oracle.pyoracle import Oracle

    return Oracle()


@pytest.mark.parametrize("sf", [7, 9, 12])
def test_reduced_column_is_the_rotated_spectrum(sf):
    """soft_bits_reduced(X) = soft_bits of the spectrum rotated by two bins, at bits 2 .. sf-1."""
    rng = np.random.default_rng(sf)
    N = 1 << sf
    for trial in range(4):
        X = (rng.standard_normal(N) + 1j * rng.standard_normal(N)).astype(np.complex64)
        if trial == 1:
            X[rng.integers(0, N, 5)] = 30.0  # equal maxima: ties give +0.0 on both sides
        if trial == 2:
            X[:] = 0
            X[N - 1] = 3.0  # the wrap: bin N - 1 rounds to value 0
        got = fs.soft_bits_reduced(X, sf)
        full = sc.soft_bits(np.roll(X, 2), sf)
        assert np.array_equal(dc.bits(got[:sf - 2]), dc.bits(full[2:])), (sf, trial)
        assert (dc.bits(got[sf - 2:]) == 0).all()
    # the hard rounding: wherever the LLR is not zero its sign is the bit of v'(argmax)
    X = (rng.standard_normal(N) + 1j * rng.standard_normal(N)).astype(np.complex64)
    for k in (N - 2, N - 1, 0, 1, 2, 4 * 5 - 1, 4 * 5 + 1, 4 * 5 + 2):
        Y = X.copy()
        Y[k] = 50.0
        llr = fs.soft_bits_reduced(Y, sf)[:sf - 2]
        v = int(fs.reduced_value(k, sf))
        assert (llr != 0).all() and np.array_equal(llr > 0, ((v >> np.arange(sf - 2)) & 1) == 1), (sf, k)


@pytest.mark.parametrize("sf", SFS)
def test_round_trip_over_the_grid(sf):
    """SF x rdd 0-4 x crc 0/1 x ten sizes (frame_checker.encode_frame's 600 cases), LLRs whose
    sign is the bit and whose magnitude is seeded uniform in 0.5 .. 1.5: the planted fields and
    payload come back, nothing corrected, no header bit flipped; without its last row the frame
    is SHORT."""
    for rdd in range(5):
        for crc in (0, 1):
            for n in sizes(sf):
                key = (sf, rdd, crc, n)
                seed = 1000 * sf + 100 * rdd + 10 * crc + n
                pay = payload_of(n, seed)
                sym = fc.encode_frame(pay, sf, rdd, crc)
                llr = fs.frame_llrs(sym, sf, np.random.default_rng(seed))
                res = fs.decode_frame_soft(llr, sf)
                assert [res[k] for k in fs.FIELDS] == [fc.OK, n, rdd, crc, len(sym), 0, 0], key
                assert res["payload"][:n].tobytes() == pay and not res["payload"][n:].any(), key
                head = fs.decode_header_soft(llr, sf)
                assert [head[k] for k in fs.FIELDS] == [fc.OK, n, rdd, crc, len(sym), 0, 0], key
                cut = fs.decode_frame_soft(llr[:-1], sf)
                assert cut["status"] == fc.SHORT and not cut["payload"].any(), key


def hard_symbols(llr, sf):
    """The symbols a hard demodulator would have given for these LLRs' signs."""
    v = ((np.asarray(llr) > 0).astype(np.int64) << np.arange(sf)[None, :]).sum(axis=1)
    sym = codes.binary_to_gray16(v.astype(np.uint16)).astype(np.int64)
    sym[:8] <<= 2
    return sym.astype(np.uint16)


@pytest.mark.parametrize("sf", SFS)
def test_soft_mends_what_hard_cannot(sf):
    """Two weak wrong bits in one Hamming 8/4 header codeword: the hard decoder raises `bad`
    (HEADER), the soft one returns the frame with hdr_flips = 2 - and refuses it at max_flips = 1."""
    rng = np.random.default_rng(40 + sf)
    n, rdd, crc = 9, 3, 1
    pay = payload_of(n, sf)
    sym = fc.encode_frame(pay, sf, rdd, crc)
    clean = fs.frame_llrs(sym, sf, rng)
    assert np.array_equal(hard_symbols(clean, sf), sym)
    for j in range(5):
        llr = clean.copy()
        for bit in rng.choice(8, 2, replace=False):
            r, c = fs.header_cell(sf, j, int(bit))
            llr[r, c] = -np.sign(llr[r, c]) * np.float32(rng.uniform(0.1, 0.4))
        assert fc.decode_frame(hard_symbols(llr, sf), sf)["status"] == fc.HEADER, j
        res = fs.decode_frame_soft(llr, sf)
        assert [res[k] for k in fs.FIELDS] == [fc.OK, n, rdd, crc, len(sym), 1, 2], j
        assert res["payload"][:n].tobytes() == pay
        tight = fs.decode_frame_soft(llr, sf, max_flips=1)
        assert [tight[k] for k in fs.FIELDS] == [fc.HEADER, 0, 0, 0, 0, 0, 2] and not tight["payload"].any()
        assert fs.decode_header_soft(llr, sf, max_flips=2)["status"] == fc.OK
    # the same in a data codeword of block 0 (SF >= 8) and of the remaining blocks (rdd 3: one bit)
    llr = clean.copy()
    r, c = 8 + 1, 3  # a cell of the first remaining block
    llr[r, c] = -np.sign(llr[r, c]) * np.float32(0.2)
    res = fs.decode_frame_soft(llr, sf)
    assert res["status"] == fc.OK and res["errors"] == 1 and res["hdr_flips"] == 0
    assert res["payload"][:n].tobytes() == pay


def test_every_other_way_a_header_is_bad():
    sf = 8
    good = fc.header_nibbles(9, 3, 1)

    def llrs(nibbles):
        cw = np.zeros(sf - 2, np.uint8)
        cw[:5] = codes.encode_hamming84(nibbles)
        sym = codes.binary_to_gray16(codes.diagonal_interleave(cw, sf - 2, 4)).astype(np.uint16) << 2
        return fs.frame_llrs(sym, sf)

    bad = {"status": fc.HEADER, "nbytes": 0, "rdd": 0, "crc": 0, "nsym": 0, "errors": 0, "hdr_flips": 0}
    assert fs.decode_header_soft(llrs(good), sf)["status"] == fc.OK
    assert fs.decode_header_soft(llrs(good[:3] + [good[3] | 2, good[4]]), sf) == bad  # nibble 3 > 1
    assert fs.decode_header_soft(llrs(good[:4] + [good[4] ^ 1]), sf) == bad           # the checksum
    for rdd in (5, 6, 7):
        h1 = (rdd << 1) | 1
        h2 = codes.header_checksum([9, h1])
        assert fs.decode_header_soft(llrs([0, 9, h1, h2 >> 4, h2 & 15]), sf) == bad, rdd
    short = dict(bad, status=fc.SHORT)
    for avail in (-1, 0, 7):
        assert fs.decode_header_soft(llrs(good), sf, avail) == short
    res = fs.decode_frame_soft(llrs(good), sf, max_bytes=20)  # 8 rows of a longer frame
    assert [res[k] for k in fs.FIELDS] == [fc.SHORT, 9, 3, 1, fc.frame_symbols(sf, 9, 3, 1), 0, 0]
    res = fs.decode_frame_soft(fs.frame_llrs(fc.encode_frame(payload_of(9, 1), sf, 3, 1), sf), sf, max_bytes=8)
    assert res["status"] == fc.SHORT and res["nbytes"] == 9 and res["payload"].shape == (8,)


def test_crc_judges_the_soft_decode():
    """rdd 0: nothing corrects a flipped data bit, the frame's checksum notices."""
    sf, n = 9, 12
    pay = payload_of(n, 3)
    sym = fc.encode_frame(pay, sf, 0, 1)
    llr = fs.frame_llrs(sym, sf, np.random.default_rng(1))
    llr[8, 0] = -llr[8, 0]
    res = fs.decode_frame_soft(llr, sf)
    assert res["status"] == fc.CRC and res["nbytes"] == n and res["errors"] == 0
    assert res["payload"][:n].tobytes() != pay


def test_ties_zeros_inf_and_nan():
    """All-zero LLRs: every metric ties at +0 and nibble 0 wins everywhere - a header of n = 0,
    rdd 0, no CRC, whose checksum (0) holds.  NaN never wins, nothing raises, no NaN comes out."""
    sf = 8
    zero = np.zeros((20, sf), np.float32)
    res = fs.decode_frame_soft(zero, sf, max_bytes=4)
    assert [res[k] for k in fs.FIELDS] == [fc.OK, 0, 0, 0, 8, 0, 0] and not res["payload"].any()
    rng = np.random.default_rng(9)
    sym = fc.encode_frame(payload_of(6, 2), sf, 2, 1)
    base = fs.frame_llrs(sym, sf, rng)
    for val in (np.nan, np.inf, -np.inf, -0.0):
        llr = base.copy()
        llr.reshape(-1)[rng.integers(0, llr.size, 12)] = np.float32(val)
        res = fs.decode_frame_soft(llr, sf)
        assert res["status"] in (fc.OK, fc.HEADER, fc.SHORT, fc.CRC)
        assert all(isinstance(res[k], int) for k in fs.FIELDS)
    # a header codeword that is all NaN: no candidate wins, nibble 0; its hard word is 0 too
    llr = base.copy()
    for bit in range(8):
        llr[fs.header_cell(sf, 0, bit)] = np.nan
    res = fs.decode_header_soft(llr, sf, max_flips=40)
    nib, cw, hard = fs.ml_decode(fs.block0_llrs(llr, sf)[:1], 4)
    assert int(nib[0]) == 0 and int(hard[0]) == 0 and res["hdr_flips"] == 0
    # +inf on one bit of a header codeword decides that bit; the lowest nibble with it wins
    L = np.zeros((1, 8), np.float32)
    L[0, 1] = np.inf
    nib, cw, hard = fs.ml_decode(L, 4)
    assert int(nib[0]) == 2 and int(hard[0]) == 2


def noisy_frame_llrs(O, sym, sf, sigma, rng):
    """([S, sf] LLRs with the header's columns reduced, the hard indices) of one modulated frame
    with white noise of `sigma` per component, on the oracle's dechirped spectra."""
    x = O.lora_modulate(np.asarray(sym, np.uint16), sf, 1, 125000, 1.0, 0x12)
    x = (x + sigma * (rng.standard_normal(len(x)) + 1j * rng.standard_normal(len(x)))).astype(np.complex64)
    X = [O.fft(w) for w in dc.frame_windows(O, x, sf, 1, "raw", False, True)]
    llr = fs.soft_bits_frame(X, sf, (2, 8))
    idx = np.array([sc.hard_index(Xs) for Xs in X], np.uint16)
    return llr[2:], idx[2:]


def test_gain_on_whole_frames(O):
    """SF 7, CR 4/5, CRC, 14 bytes, noise_sigma(-7.0), 300 frames from default_rng(7); a frame is
    wrong unless its status is OK and its payload exact.  The soft decoder (max_flips 5) loses at
    most half the frames the hard one loses.  The checker's counts on the oracle's kissfft-ordered
    fp32 spectra: hard 161, soft 50 (the float64-FFT model gave 153 and 54)."""
    sf, rdd, F, n = 7, 1, 300, 14
    rng = np.random.default_rng(7)
    sigma = sc.noise_sigma(-7.0)
    hard_bad = soft_bad = 0
    for f in range(F):
        pay = rng.integers(0, 256, n).astype(np.uint8)
        sym = fc.encode_frame(pay.tobytes(), sf, rdd, 1)
        llr, idx = noisy_frame_llrs(O, sym, sf, sigma, rng)
        h = fc.decode_frame(idx, sf, max_bytes=n)
        s = fs.decode_frame_soft(llr, sf, max_bytes=n)
        hard_bad += not (h["status"] == fc.OK and np.array_equal(h["payload"], pay))
        soft_bad += not (s["status"] == fc.OK and np.array_equal(s["payload"], pay))
    print(f"hard_bad={hard_bad} soft_bad={soft_bad} of {F}")
    assert hard_bad >= 30
    assert 2 * soft_bad <= hard_bad


def test_header_gate_on_noise(O):
    """20,000 seeded noise-only headers at SF 7 (eight windows of unit white noise each): how many
    pass the hard gate, and the soft gate at max_flips 40 and 5.  The limit is what keeps the soft
    gate as tight as the hard one: pass(5) < pass(40) and pass(5) <= 10, twice the worst figure of
    the hard gate on record (2 to 5 per 20,000).  Counts on the oracle's spectra: hard 3, soft at
    max_flips 40: 57, soft at max_flips 5: 5 (the float64-FFT model gave 5, 54 and 0)."""
    sf, H = 7, 20000
    N = 1 << sf
    rng = np.random.default_rng(11)
    hard = soft40 = soft5 = 0
    for h in range(H):
        w = (rng.standard_normal((8, N)) + 1j * rng.standard_normal((8, N))).astype(np.complex64)
        X = [O.fft(ws) for ws in w]
        llr = np.stack([fs.soft_bits_reduced(Xs, sf) for Xs in X])
        idx = np.array([sc.hard_index(Xs) for Xs in X], np.uint16)
        hard += fc.decode_header(idx, sf)["status"] == fc.OK
        wide = fs.decode_header_soft(llr, sf, max_flips=40)
        soft40 += wide["status"] == fc.OK
        soft5 += wide["status"] == fc.OK and wide["hdr_flips"] <= 5
    print(f"noise headers passed of {H}: hard {hard}, soft(40) {soft40}, soft(5) {soft5}")
    assert soft5 < soft40
    assert soft5 <= 10
