"""CPU: the soft-decision definitions (include/lora_mi355x.h, lora_demod_soft_bits_batch and
lora_decode_chain_soft_batch) as tests/soft_checker.py restates them: consistent with the
hard path wherever they must be, correcting what a hard decoder cannot, and worth about as
much at the waterfall as the model that motivated them.  The kernels are compared with the
same checker bit for bit in tests/test_gpu_soft.py."""
import numpy as np
import pytest

from lora_phy_amd import codes
from tests import detect_checker as dc
from tests import soft_checker as sc

NOISY_DB = {6: -6.0, 7: -8.0, 9: -14.0}  # soft_checker.noise_sigma's labels: some symbols fail


@pytest.fixture(scope="module")
def O():
    from oracle.pyoracle import Oracle

    return Oracle()


def spectra(O, x, sf):
    """[total, N] spectra of one dechirped frame, as a raw plan with dechirp feeds them."""
    return [O.fft(w) for w in dc.frame_windows(O, x, sf, 1, "raw", False, True)]


@pytest.mark.parametrize("rdd", [1, 4])
@pytest.mark.parametrize("sf", [6, 7, 9])
def test_soft_bits_agree_with_the_hard_path(O, sf, rdd):
    nbytes = 9
    rng = np.random.default_rng(100 * sf + rdd)
    pay = rng.integers(0, 256, (2, nbytes)).astype(np.uint8)
    for snr in (None, NOISY_DB[sf]):
        x = sc.chain_frames(O, sf, rdd, pay, snr, rng)
        wrong = 0
        for f in range(len(pay)):
            X = spectra(O, x[f], sf)
            llr = np.stack([sc.soft_bits(Xs, sf) for Xs in X])
            idx = np.array([dc.detect(Xs)[0] for Xs in X], np.uint16)
            assert np.array_equal(idx, [sc.hard_index(Xs) for Xs in X])
            assert not np.isnan(llr).any()
            v = codes.gray_to_binary16(idx).astype(np.int64)
            bit = (v[:, None] >> np.arange(sf)[None, :]) & 1
            nz = llr != 0
            assert nz.mean() > 0.9  # a tie of two maxima is the exception
            assert np.array_equal((llr > 0)[nz], bit[nz] == 1)
            # rdd 0: the signs alone, so the hard chain's payload on the same indices
            n0 = (len(idx) - 2) // 4 * sf // 2
            soft0, corr0 = sc.decode_chain_soft(llr[2:], sf, 0, n0)
            if nz.all():
                assert np.array_equal(soft0, codes.decode_chain(idx[2:], sf, 0, n0)["payload"])
            assert corr0 == 0
            got, _ = sc.decode_chain_soft(llr[2:], sf, rdd, nbytes)
            if snr is None:
                assert np.array_equal(got, pay[f])
                for r in range(5):  # noiseless: the payload at every rdd
                    xr = sc.chain_frames(O, sf, r, pay[f:f + 1])[0]
                    lr = np.stack([sc.soft_bits(Xs, sf) for Xs in spectra(O, xr, sf)])
                    gr, cr = sc.decode_chain_soft(lr[2:], sf, r, nbytes)
                    assert np.array_equal(gr, pay[f]) and cr == 0, r
            else:
                wrong += int((idx[2:] != codes.encode_chain(pay[f].tobytes(), sf, rdd)["symbols"]).sum())
        if snr is not None:
            assert wrong > 0, "the noisy case must contain symbol errors"


def pm_one(symbols, sf):
    """+-1 LLRs of the chain's symbols: the sign is the bit of grayToBinary16(symbol)."""
    v = codes.gray_to_binary16(np.asarray(symbols, np.uint16)).astype(np.int64)
    return np.where(((v[:, None] >> np.arange(sf)[None, :]) & 1) == 1, 1.0, -1.0).astype(np.float32)


def flip_one_per_codeword(llr, sf, rdd, rng, scale=-1.0):
    """Multiply one LLR of every codeword by ``scale`` (through the deinterleave map)."""
    nb = 4 + rdd
    out = llr.copy()
    for j in range(llr.shape[0] // nb * sf):
        blk, dst = divmod(j, sf)
        bit = int(rng.integers(0, nb))
        out[blk * nb + bit, (dst - bit) % sf] *= np.float32(scale)
    return out


@pytest.mark.parametrize("sf", [7, 10])
def test_one_flip_per_codeword_is_corrected_at_every_code_rate(sf):
    rng = np.random.default_rng(sf)
    nbytes = 13
    pay = rng.integers(0, 256, nbytes).astype(np.uint8)
    for rdd in range(1, 5):
        syms = codes.encode_chain(pay.tobytes(), sf, rdd)["symbols"]
        clean = pm_one(syms, sf)
        got, corr = sc.decode_chain_soft(clean, sf, rdd, nbytes)
        assert np.array_equal(got, pay) and corr == 0
        # a full sign flip: the metric of the sent codeword is nb - 2, every other one's at most
        # nb - 2 d_min + 2 - except at rdd 1 and 2 (d_min 2), where a full flip ties and only a
        # weaker wrong bit can be outvoted: flips of magnitude 0.5 there
        weak = np.float32(-0.5)
        bad = flip_one_per_codeword(clean, sf, rdd, rng, -1.0 if rdd >= 3 else weak)
        got, corr = sc.decode_chain_soft(bad, sf, rdd, nbytes)
        assert np.array_equal(got, pay), rdd
        assert corr == 2 * nbytes, rdd  # every codeword among the first 2 nbytes was flipped
        # the hard decoder on the same signs
        v = ((bad > 0).astype(np.int64) << np.arange(sf)[None, :]).sum(axis=1)
        hard = codes.decode_chain(codes.binary_to_gray16(v.astype(np.uint16)), sf, rdd, nbytes)["payload"]
        assert np.array_equal(hard, pay) == (rdd >= 3), rdd


def test_half_magnitude_flips_are_counted():
    sf, rdd, nbytes = 8, 1, 6
    rng = np.random.default_rng(3)
    pay = rng.integers(0, 256, nbytes).astype(np.uint8)
    llr = pm_one(codes.encode_chain(pay.tobytes(), sf, rdd)["symbols"], sf)
    nb = 4 + rdd
    flipped = [0, 3, 4, 11, 13]  # 13 is beyond the first 2 * nbytes = 12 codewords
    for j in flipped:
        blk, dst = divmod(j, sf)
        llr[blk * nb + 2, (dst - 2) % sf] *= np.float32(-0.5)
    got, corr = sc.decode_chain_soft(llr, sf, rdd, nbytes)
    assert np.array_equal(got, pay)
    assert corr == sum(j < 2 * nbytes for j in flipped) == 4


def test_ties_nan_and_inf_follow_the_scan_rule():
    sf, rdd = 7, 1
    llr = np.zeros((5, sf), np.float32)  # one block, all +0: every metric ties at +0
    pay, corr = sc.decode_chain_soft(llr, sf, rdd, 3)
    assert pay.tolist() == [0, 0, 0] and corr == 0
    llr[0, 0] = np.nan  # codeword 0, bit 0: all its metrics are NaN, none wins, nibble 0
    llr[1, 0] = np.inf  # codeword 1, bit 1 = +inf
    w = np.frombuffer(codes.sx1272_whitening_lfsr(bytes(sf), 0, rdd), np.uint8)
    pay, _ = sc.decode_chain_soft(llr, sf, rdd, 3)
    assert pay[0] >> 4 == 0
    want = 0 if (w[1] >> 1) & 1 else 2  # the sign the whitening leaves; then the lowest nibble with that bit
    assert pay[0] & 0xF == want


def test_gain_at_the_waterfall(O):
    """SF 7, CR 4/5, -7 dB (noise_sigma: sigma = 10^(-snr/20) per component, the figure of the
    model that motivated the soft path), 300 seeded frames of 16 bytes: the soft decoder loses
    at most half the frames the hard one loses.  The checker's counts on kissfft-ordered fp32
    spectra: hard 166, soft 44 (the float64-FFT model gave 158 and 49)."""
    sf, rdd, F, nbytes = 7, 1, 300, 16
    rng = np.random.default_rng(7)
    pay = rng.integers(0, 256, (F, nbytes)).astype(np.uint8)
    x = sc.chain_frames(O, sf, rdd, pay, -7.0, rng)
    llr, idx = sc.soft_bits_frames(O, x, sf, 1, "raw", False, True, with_index=True)
    hard_bad = soft_bad = 0
    for f in range(F):
        hard_bad += not np.array_equal(codes.decode_chain(idx[f, 2:], sf, rdd, nbytes)["payload"], pay[f])
        soft_bad += not np.array_equal(sc.decode_chain_soft(llr[f, 2:], sf, rdd, nbytes)[0], pay[f])
    print(f"hard_bad={hard_bad} soft_bad={soft_bad} of {F}")
    assert hard_bad >= 30
    assert 2 * soft_bad <= hard_bad
