"""CPU: the host model of the wideband transmit side (tests/synth_checker.py).

``synthesize_host`` against a float64 evaluation of the direct zero-stuffed form, the raw store
rule against ``raw_to_complex``'s arithmetic, the chunking rule, and the loop-back on the host:
planted channel streams -> ``synthesize_host`` -> noise -> ``channel_checker.channelize_host`` ->
the scan checker's finder -> the oracle's demodulator, which must return every planted frame of
every channel where the two delays put it."""
import numpy as np
import pytest

from tests import channel_checker as cc
from tests import scan_checker as sc
from tests import synth_checker as sy


@pytest.fixture(scope="module")
def O():
    from oracle.pyoracle import Oracle

    return Oracle()


def noise(shape, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


@pytest.mark.parametrize("T,U,period,steps,gains,Lc", [
    (7, 3, 5, (-2, 0, 7), (1.0, -0.5, 0.1), 60), (65, 8, 5, (-2, -1, 0, 1, 2), None, 90),
    (33, 4, 64, tuple(range(-9, 9)), None, 50), (3, 8, 4, (1,), (2.0,), 20), (12, 1, 7, (3, 4), (0.0, 1.5), 40)])
def test_host_model_agrees_with_a_float64_evaluation(T, U, period, steps, gains, Lc):
    """Every term of an output, h * g * x * w, passes through at most n = P + C + 4 roundings:
    the gain, the tap's product, at most P running sums, one product and one sum of the mix, at
    most C sums over the channels.  So the error is at most gamma_n = n u / (1 - n u), u = 2^-24,
    times the sum of the terms' magnitudes, which synthesize_f64(magnitudes=True) evaluates with
    |w's components| <= 1; the float64 evaluation's own error is below 2^-40 of the same sum."""
    C = len(steps)
    x, h = noise((C, Lc), T * 100 + U), np.random.default_rng(T).standard_normal(T).astype(np.float32)
    got = sy.synthesize_host(x, h, U, steps, period, gains, first_sample=11)
    want = sy.synthesize_f64(x, h, U, steps, period, gains, first_sample=11)
    mag = sy.synthesize_f64(x, h, U, steps, period, gains, magnitudes=True)
    assert got.shape == want.shape == mag.shape == (sy.outputs(Lc, T, U),) and got.shape[0] > 0
    n, u = sy.phases(T, U) + C + 4, 2.0 ** -24
    bound = (n * u / (1 - n * u) + 2.0 ** -40) * mag
    err = np.maximum(np.abs(got.real - want.real), np.abs(got.imag - want.imag))
    assert (err <= bound).all(), (float((err - bound).max()), float(bound.max()))
    assert err.max() > 0  # (fp32 roundings are really there: the comparison is not vacuous)


def test_output_count_shapes_and_delay():
    for T, U in ((7, 3), (65, 8), (2, 8), (1, 1), (512, 64), (8, 8), (9, 8)):
        P = -(-T // U)
        assert sy.phases(T, U) == P
        for Lc, W in ((0, 0), (P - 1, 0), (P, U), (P + 1, 2 * U), (P + 10, 11 * U)):
            if Lc >= 0:
                assert sy.outputs(Lc, T, U) == W
        assert sy.delay(T, U) == (T - 1) / 2 - (P - 1) * U
    assert sy.synthesize_host(np.zeros((2, 2), np.complex64), np.ones(7), 3, (0, 1), 4).shape == (0,)
    assert sy.synthesize_host(np.zeros((3, 2, 5), np.complex64), np.ones(7), 3, (0, 1), 4).shape == (3, 9)
    assert sy.delay(65, 8) == -32.0 and sy.loopback_shift(65, 8, 65, 8) == -8 and sy.loopback_shift(33, 8, 33, 8) == -4


def test_an_impulse_comes_out_as_the_taps_around_its_delay():
    """One unit sample at m: the outputs are the taps, tap j at output m*U - (P-1)*U + j, so the
    filter's centre (ntaps-1)/2 is at m*U + delay; and phases with K == 0 give +0."""
    T, U, Lc, m = 11, 4, 12, 5
    h = np.arange(1, T + 1, dtype=np.float32)
    x = np.zeros((1, Lc), np.complex64)
    x[0, m] = 1
    y = sy.synthesize_host(x, h, U, (0,), 1)
    first = m * U - (sy.phases(T, U) - 1) * U
    assert np.array_equal(y[first:first + T], h.astype(np.complex64))
    assert not y[:first].any() and not y[first + T:].any()
    assert first + (T - 1) / 2 == m * U + sy.delay(T, U)
    y = sy.synthesize_host(np.ones((1, 4), np.complex64), [2.0, 3.0], 4, (0,), 1)   # ntaps < interp
    assert np.array_equal(y.view(np.uint32).reshape(-1, 2)[:4], np.array(
        [[np.float32(v).view(np.uint32), 0] for v in (2.0, 3.0, 0.0, 0.0)], np.uint32))


def test_a_second_chunk_with_first_sample_continues_the_first():
    T, U, period, steps, gains = 33, 4, 7, (-3, 1, 2), (1.0, 0.5, -2.0)
    x, h = noise((3, 200), 5), sy.lowpass_taps(T, 0.5 / U, U)
    P = sy.phases(T, U)
    whole = sy.synthesize_host(x, h, U, steps, period, gains)
    n1 = 90  # channel samples in the first chunk
    first = sy.synthesize_host(x[:, :n1], h, U, steps, period, gains)
    second = sy.synthesize_host(x[:, n1 - (P - 1):], h, U, steps, period, gains, first_sample=len(first))
    assert len(first) + len(second) == len(whole)
    assert np.array_equal(np.concatenate([first, second]).view(np.uint32), whole.view(np.uint32))
    assert not np.array_equal(sy.synthesize_host(x[:, n1 - (P - 1):], h, U, steps, period, gains), whole[len(first):])


@pytest.mark.parametrize("dtype", [np.int16, np.int8, np.uint8])
def test_store_round_trips_every_code(dtype):
    """raw_to_complex's arithmetic, x = (float(v) - bias) * scale with the default scale, then the
    store rule with the default inv_scale: every code of the format comes back."""
    default, bias, lo, hi, zero = sy.RAW[np.dtype(dtype)]
    codes = np.arange(lo, hi + 1, dtype=np.int64)
    scale = np.float32(1.0 / default)
    x = ((codes.astype(np.float32) - np.float32(bias)).astype(np.float32) * scale).astype(np.float32)
    y = (x + 1j * x[::-1]).astype(np.complex64)
    got = sy.store_host(y, dtype)
    assert got.dtype == np.dtype(dtype) and got.shape == (len(codes), 2)
    assert np.array_equal(got[:, 0].astype(np.int64), codes) and np.array_equal(got[:, 1].astype(np.int64), codes[::-1])


def test_store_saturates_rounds_ties_to_even_and_zeroes_nan():
    inf, nan = np.inf, np.nan
    y = np.array([complex(2.0, -2.0), complex(inf, -inf), complex(nan, 0.0), complex(0.5 / 128, 1.5 / 128),
                  complex(2.5 / 128, -0.5 / 128), complex(-1.5 / 128, -2.5 / 128)], np.complex64)
    assert sy.store_host(y, np.int8).tolist() == [[127, -128], [127, -128], [0, 0], [0, 2], [2, 0], [-2, -2]]
    assert sy.store_host(y[:3], np.int16).tolist() == [[32767, -32768], [32767, -32768], [0, 0]]
    # cu8: v = y * 127.5 + 127.5, so y = k / 127.5 is a tie: 0 -> 127.5 -> 128 (even), -1/127.5 -> 126
    t = np.array([complex(0.0, -1.0 / 127.5), complex(2.0, -2.0), complex(nan, inf)], np.complex64)
    assert sy.store_host(t, np.uint8).tolist() == [[128, 126], [255, 0], [128, 255]]
    assert sy.store_host(np.array([1.0 + 0.5j], np.complex64), np.int16, inv_scale=100.0).tolist() == [[100, 50]]


LOOPBACK = [(ci, ai, sigma) for ci in (0, 2, 3) for ai in range(len(cc.CONFIGS[ci][8])) for sigma in (0.0, 0.1)]


def loopback_signal(O, ci: int, ai: int, sigma: float):
    """(x complex64 [W], planted, synthesis taps): configuration ci's planted channels through
    synthesize_host with the amps variant ai as gains and edge-cutoff taps, plus
    channel_checker.wideband's noise."""
    sf, osr, D, period, T, cutoff, rows, steps, amps = cc.CONFIGS[ci]
    chans, planted = sy.planted_channels(O, ci)
    h = sy.lowpass_taps(T, 0.5 / D, gain=D)
    x = sy.synthesize_host(chans, h, D, steps, period, amps[ai])
    if sigma:
        rng = np.random.default_rng(cc.SEED0 + 99)
        x = (x + sigma * (rng.standard_normal(len(x)) + 1j * rng.standard_normal(len(x)))).astype(np.complex64)
    return x, planted, h


@pytest.mark.parametrize("ci,ai,sigma", LOOPBACK)
def test_every_planted_frame_comes_back_through_both_banks_on_the_host(O, ci, ai, sigma):
    sf, osr, D, period, T, cutoff, rows, steps, amps = cc.CONFIGS[ci]
    x, planted, _ = loopback_signal(O, ci, ai, sigma)
    rows_out = cc.channelize_host(x, cc.lowpass_taps(T, cutoff), steps, period, D)
    step = (1 << sf) * osr
    hop = step // 4
    shift = sy.loopback_shift(T, D, T, D)
    for c, (starts, syms) in enumerate(planted):
        S = syms.shape[1]
        y = rows_out[c]
        found = sc.find_frames_host(sc.scan_host(O, y, sf, osr, hop, dechirp=True), hop, sf, osr, S, 0x12,
                                    row_len=len(y))
        assert found.tolist() == (starts + shift).tolist(), (c, found, starts + shift)
        frame_len = (S + 2) * step
        cut = np.stack([y[s:s + frame_len] for s in found])
        o_syms, o_sync, _, _, cnt = O.demod_frames(cut, sf, osr, False, True)
        assert (np.asarray(cnt) == S).all()
        assert np.array_equal(np.asarray(o_syms)[:, :S] % (1 << sf), syms), c
        assert (np.asarray(o_sync) == 0x12).all(), c
