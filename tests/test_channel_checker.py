"""CPU: the host model of the wideband front end (tests/channel_checker.py).

``channelize_host`` against a float64 evaluation of the same sums, the ``first_sample`` chunking
rule, and the whole receive chain on the host: ``wideband`` -> ``channelize_host`` ->
``scan_checker.scan_host`` -> ``find_frames_host`` -> the oracle's demodulator, which must return
every planted frame of every channel where the channelizer's delay puts it."""
import numpy as np
import pytest

from tests import channel_checker as cc
from tests import scan_checker as sc


@pytest.fixture(scope="module")
def O():
    from oracle.pyoracle import Oracle

    return Oracle()


@pytest.mark.parametrize("T,D,period,steps,L", [(7, 3, 5, (-2, 0, 7), 100), (65, 8, 5, (-2, -1, 0, 1, 2), 700),
                                                (33, 4, 64, tuple(range(-9, 9)), 300), (3, 8, 4, (1,), 64)])
def test_host_model_agrees_with_a_float64_evaluation(T, D, period, steps, L):
    """Each output is a sum of T products h[j] * z with |z| <= (1 + 3 eps) sqrt(2) |x|: the mixing
    costs 3 roundings, each tap one for its product and one for the running sum, whose partial
    sums stay below sum|h| max|z|.  8 eps32 T sum|h| max|x| covers that with room (the bound the
    GPU tests' reference is held to)."""
    rng = np.random.default_rng(T * 100 + D)
    x = (rng.standard_normal(L) + 1j * rng.standard_normal(L)).astype(np.complex64)
    h = rng.standard_normal(T).astype(np.float32)
    got = cc.channelize_host(x, h, steps, period, D, first_sample=11)
    want = cc.channelize_f64(x, h, steps, period, D, first_sample=11)
    assert got.shape == want.shape == (len(steps), cc.outputs(L, T, D)) and got.shape[1] > 0
    bound = 8 * np.finfo(np.float32).eps * T * np.abs(h).sum() * np.abs(x).max()
    err = max(np.abs(got.real - want.real).max(), np.abs(got.imag - want.imag).max())
    assert err <= bound, (err, bound)
    assert err > 0  # (fp32 roundings are really there: the comparison is not vacuous)


def test_output_count_and_shapes():
    T, D = 7, 3
    for L, W in ((0, 0), (T - 1, 0), (T, 1), (T + D - 1, 1), (T + D, 2)):
        assert cc.outputs(L, T, D) == W
        assert cc.channelize_host(np.zeros(L, np.complex64), np.ones(T), (0, 1), 4, D).shape == (2, W)
    assert cc.channelize_host(np.zeros((3, 20), np.complex64), np.ones(T), (0, 1), 4, D).shape == (3, 2, 5)


def test_one_tap_no_decimation_is_a_scaled_copy():
    x = (np.arange(17) + 1j * np.arange(17)[::-1]).astype(np.complex64)
    got = cc.channelize_host(x, [0.5], (0,), 1, 1)
    assert np.array_equal(got[0], (0.5 * x).astype(np.complex64))


def test_a_second_chunk_with_first_sample_continues_the_first():
    """A chunk that starts at a multiple of decim, run with first_sample, equals the matching
    columns of the whole run, bit for bit; chunks overlapping by ntaps - decim tile the outputs."""
    T, D, period, steps = 33, 4, 7, (-3, 1, 2)
    rng = np.random.default_rng(5)
    x = (rng.standard_normal(900) + 1j * rng.standard_normal(900)).astype(np.complex64)
    h = cc.lowpass_taps(T, 0.2)
    whole = cc.channelize_host(x, h, steps, period, D)
    t1 = 100  # the second chunk's first output
    first = cc.channelize_host(x[:(t1 - 1) * D + T], h, steps, period, D)
    second = cc.channelize_host(x[t1 * D:], h, steps, period, D, first_sample=t1 * D)
    assert first.shape[1] == t1 and first.shape[1] + second.shape[1] == whole.shape[1]
    assert ((t1 - 1) * D + T) - t1 * D == T - D  # the overlap
    assert np.array_equal(first.view(np.uint32), whole[:, :t1].view(np.uint32))
    assert np.array_equal(second.view(np.uint32), whole[:, t1:].view(np.uint32))
    # without first_sample the oscillator restarts and the chunk differs
    assert not np.array_equal(cc.channelize_host(x[t1 * D:], h, steps, period, D), whole[:, t1:])


CASES = [(ci, ai, sigma) for ci, cfg in enumerate(cc.CONFIGS) for ai in range(len(cfg[8])) for sigma in (0.0, 0.1)]


@pytest.mark.parametrize("ci,ai,sigma", CASES)
def test_every_planted_frame_of_every_channel_is_received_on_the_host(O, ci, ai, sigma):
    sf, osr, D, period, T, cutoff, rows, steps, amps = cc.CONFIGS[ci]
    x, planted, taps = cc.config_signal(O, ci, ai, sigma)
    rows_out = cc.channelize_host(x, taps, steps, period, D)
    step = (1 << sf) * osr
    hop = step // 4
    shift = (T - 1) // 2 // D  # the delay in channel samples
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
