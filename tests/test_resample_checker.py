"""CPU: the host model of the rational-rate bank (tests/resample_checker.py).

``resample_host`` against the integer bank's model at interp 1, against the direct zero-stuffed
form in float64, its exact zeros and its output count; and the whole receive chain on the host:
``wideband`` -> ``resample_host`` -> ``scan_checker.scan_host`` -> ``find_frames_host`` -> the
oracle's demodulator, which must return every planted frame of every channel where the bank's
delay puts it.  The GPU tests ask for what this host run gives."""
import numpy as np
import pytest

from tests import channel_checker as cc
from tests import resample_checker as rc
from tests import scan_checker as sc
from tests.test_gpu_channelize import SHAPES as INTEGER_SHAPES


@pytest.fixture(scope="module")
def O():
    from oracle.pyoracle import Oracle

    return Oracle()


def noise(shape, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


def bits(a):
    return np.ascontiguousarray(a, np.complex64).view(np.uint32)


@pytest.mark.parametrize("T,D,period,steps,L", [s[:5] for s in INTEGER_SHAPES if s[4] <= 700])
def test_interp_one_is_the_integer_bank_bit_for_bit(T, D, period, steps, L):
    x = noise(L, 100 + T + L)
    h = np.random.default_rng(T).standard_normal(T).astype(np.float32)
    assert rc.outputs(L, T, 1, D) == cc.outputs(L, T, D)
    got = rc.resample_host(x, h, steps, period, 1, D, first_sample=7)
    want = cc.channelize_host(x, h, steps, period, D, first_sample=7)
    assert got.shape == want.shape and got.shape[1] > 0
    assert np.array_equal(bits(got), bits(want))


def test_interp_one_counts_outputs_as_the_integer_bank():
    for T, D in ((7, 3), (1, 1), (65, 8)):
        for L in range(0, 3 * T + 2 * D):
            assert rc.outputs(L, T, 1, D) == cc.outputs(L, T, D)


# (interp, decim, ntaps, row_len): the polyphase indexing against the direct form, ntaps < interp
# and W = 1 included
FORMS = [(1, 8, 65, 300), (2, 5, 41, 200), (3, 8, 49, 333), (5, 96, 385, 2000), (4, 7, 3, 50), (7, 9, 1, 40),
         (3, 4, 2, 10), (2, 3, 5, 3), (16, 256, 4096, 700)]


@pytest.mark.parametrize("Li,D,T,L", FORMS)
def test_host_model_agrees_with_the_direct_form_in_float64(Li, D, T, L):
    """Output t sums K products h[j0 + i*Li] * z with |z| <= (1 + 3 eps) sqrt(2) |x|: the mixing
    costs 3 roundings, each tap one for its product and one for the running sum, whose partial sums
    stay below sum|h_r| max|z| (h_r: the residue's sub-filter).  (3 + 2 K) sqrt(2) <= 8 K for K >=
    1, so 8 eps32 K sum|h_r| max|x| covers it, per residue; the direct form's own error in double
    is 2^-29 of that."""
    period, steps = 12, (-2, 0, 5)
    x = noise(L, Li * 1000 + D)
    h = np.random.default_rng(T).standard_normal(T).astype(np.float32)
    got = rc.resample_host(x, h, steps, period, Li, D, first_sample=11)
    want = rc.resample_f64(x, h, steps, period, Li, D, first_sample=11)
    W = rc.outputs(L, T, Li, D)
    assert got.shape == want.shape == (len(steps), W) and W > 0
    eps = np.finfo(np.float32).eps
    worst = 0.0
    for r in range(min(Li, W)):
        j0, off, K = rc.residue(r, T, Li, D)
        g, w = got[:, r::Li], want[:, r::Li]
        err = max(np.abs(g.real - w.real).max(), np.abs(g.imag - w.imag).max())
        if K == 0:
            assert err == 0 and (w == 0).all()
            continue
        bound = 8 * eps * K * np.abs(h[j0::Li]).sum() * np.abs(x).max()
        assert err <= bound, (r, err, bound)
        worst = max(worst, err)
    assert worst > 0 or T == 1  # (fp32 roundings are really there: the comparison is not vacuous)


def test_a_residue_without_a_tap_gives_positive_zero():
    """interp 3, decim 4, two taps: t = 1 (mod 3) has j0 = 2 >= ntaps, K = 0."""
    Li, D, T = 3, 4, 2
    assert [rc.residue(r, T, Li, D) for r in range(3)] == [(0, 0, 1), (2, 2, 0), (1, 3, 1)]
    x = noise(40, 1)
    x[5] = complex(-0.0, np.nan)  # nothing of the input reaches an output without a tap
    got = rc.resample_host(x, [-1.5, 2.0], (1, -1), 5, Li, D)
    assert got.shape[1] >= 6
    assert (bits(got[:, 1::3]) == 0).all()  # +0.0f, not -0.0f
    assert (bits(got[:, 0::3]) != 0).all() and (bits(got[:, 2::3]) != 0).all()


def test_output_count_around_one_output():
    for Li, D, T in ((2, 3, 5), (3, 8, 49), (5, 96, 385), (3, 4, 2), (1, 3, 7)):
        first = -(-(T - 1) // Li) + 1                 # the shortest row with an output: span >= ntaps
        second = -(-(T - 1 + D) // Li) + 1            # .. with two: span >= ntaps + decim
        table = [(0, 0), (first - 1, 0), (first, 1), (second - 1, 1), (second, 2)]
        for L, W in table:
            if L >= 0:
                assert rc.outputs(L, T, Li, D) == W, (Li, D, T, L)
                got = rc.resample_host(np.zeros(L, np.complex64), np.ones(T), (0, 1), 4, Li, D)
                assert got.shape == (2, W)
    assert rc.outputs(3, 5, 2, 3) == 1 and rc.outputs(2, 5, 2, 3) == 0
    assert rc.resample_host(np.zeros((3, 20), np.complex64), np.ones(5), (0, 1), 4, 2, 3).shape == (3, 2, 12)


def test_a_second_chunk_with_first_sample_continues_the_first():
    """A chunk that starts at n0 with n0 * interp a multiple of decim, run with first_sample = n0,
    equals the columns of the whole run from n0 * interp / decim on, bit for bit."""
    Li, D, T, period, steps = 3, 8, 49, 7, (-3, 1, 2)
    x = noise(900, 5)
    h = rc.lowpass_taps(T, 0.5 / D, gain=Li)
    whole = rc.resample_host(x, h, steps, period, Li, D)
    n0 = 8 * 30  # n0 * 3 / 8 = 90 outputs before it
    t1 = n0 * Li // D
    short = -(-((t1 - 1) * D + T - 1) // Li) + 1  # the shortest predecessor that holds t1 outputs
    first = rc.resample_host(x[:short], h, steps, period, Li, D)
    second = rc.resample_host(x[n0:], h, steps, period, Li, D, first_sample=n0)
    assert first.shape[1] == t1 and first.shape[1] + second.shape[1] == whole.shape[1]
    assert np.array_equal(bits(first), bits(whole[:, :t1]))
    assert np.array_equal(bits(second), bits(whole[:, t1:]))
    assert not np.array_equal(rc.resample_host(x[n0:], h, steps, period, Li, D), whole[:, t1:])


def test_lowpass_taps_gain_is_applied_in_double():
    from lora_phy_amd import stream

    for T, cutoff, gain in ((41, 0.1, 2), (385, 0.5 / 96, 5), (49, 0.0625, 3.0), (65, 0.1, 1.0)):
        h = stream.lowpass_taps(T, cutoff, gain=gain)
        assert h.dtype == np.float32 and np.array_equal(h, rc.lowpass_taps(T, cutoff, gain))
        assert abs(float(h.astype(np.float64).sum()) - gain) < 1e-6 * gain
    assert np.array_equal(stream.lowpass_taps(65, 0.1), cc.lowpass_taps(65, 0.1))
    assert np.array_equal(stream.lowpass_taps(65, 0.1, gain=1.0), stream.lowpass_taps(65, 0.1))


CASES = [(ci, sigma) for ci in range(len(rc.CONFIGS)) for sigma in rc.SIGMAS]


@pytest.mark.parametrize("ci,sigma", CASES)
def test_every_planted_frame_of_every_channel_is_received_on_the_host(O, ci, sigma):
    sf, osr, Li, D, period, T, rows, steps, amps = rc.CONFIGS[ci]
    x, planted, taps = rc.config_signal(O, ci, sigma)
    rows_out = rc.resample_host(x, taps, steps, period, Li, D)
    step = (1 << sf) * osr
    hop = step // 4
    shift = (T - 1) // (2 * D)  # the delay in channel samples
    for c, (starts, syms) in enumerate(planted):
        S = syms.shape[1]
        y = rows_out[c]
        found = sc.find_frames_host(sc.scan_host(O, y, sf, osr, hop, dechirp=True), hop, sf, osr, S, 0x12,
                                    row_len=len(y))
        assert found.tolist() == (starts - shift).tolist(), (c, found, starts - shift)
        frame_len = (S + 2) * step
        cut = np.stack([y[s:s + frame_len] for s in found])
        o_syms, o_sync, _, _, cnt = O.demod_frames(cut, sf, osr, False, True)
        assert (np.asarray(cnt) == S).all()
        assert np.array_equal(np.asarray(o_syms)[:, :S] % (1 << sf), syms), c
        assert (np.asarray(o_sync) == 0x12).all(), c
