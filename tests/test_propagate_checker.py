"""CPU: the propagation stage's host restatement (tests/propagate_checker.py) and the default
fractional-delay table: the table's rows, its worst-case response error against the figure the
beta sweep recorded, a whole-sample delay as a copy, chunking, the
rotation against the impairment stage's, and the 64-bit triangle number.

Only the table tests, the word helpers and ``test_the_entry_exists`` touch the library.  The
others hold the checker to itself, to ``impair_checker`` and to Python integers: they make the
checker a reference worth comparing with and say nothing about the stage, whose coverage is
tests/test_gpu_propagate.py."""
import numpy as np
import pytest

from lora_phy_amd import _capi, stream
from tests import impair_checker as ic
from tests import propagate_checker as pc

# the smallest worst-case error of the sweep over beta at 16 taps, at
# beta = 5.05, on 1601 frequencies in |f| <= 0.4
RECORDED_ERROR = 4.753e-3


def rows(R, L, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((R, L)) + 1j * rng.standard_normal((R, L))).astype(np.complex64)


def bits(z):
    return np.ascontiguousarray(z, np.complex64).view(np.uint32)


def test_the_entry_exists():
    assert "lora_propagate_batch" in _capi.EXPORTED_SYMBOLS and hasattr(_capi.lib(), "lora_propagate_batch")


@pytest.mark.parametrize("taps", [2, 16, 32])
def test_table_rows(taps):
    tab = stream.fracdelay_table(taps)
    assert tab.dtype == np.float32 and tab.shape == (256, taps)
    assert np.array_equal(tab.view(np.uint32), pc.fracdelay_table(taps).view(np.uint32))
    impulse = np.zeros(taps, np.float32)
    impulse[taps // 2 - 1] = 1.0
    assert np.array_equal(tab[0].view(np.uint32), impulse.view(np.uint32))
    # every row sums to 1 within the roundings of its entries: half an ulp of each
    slack = np.spacing(np.abs(tab)).astype(np.float64).sum(axis=1) / 2
    assert np.all(np.abs(tab.astype(np.float64).sum(axis=1) - 1.0) <= slack)


def test_default_table_response_error():
    assert stream.FRACDELAY_BETA == 5.05
    err = pc.response_error(stream.fracdelay_table(), fmax=0.4, points=1601)
    print("worst-case response error", err)
    assert err <= 2 * RECORDED_ERROR
    # and the sweep's choice is a minimum of the sweep: its neighbours are no better
    for beta in (4.8, 5.3):
        assert pc.response_error(stream.fracdelay_table(16, beta), points=1601) > err


def test_word_helpers_agree_with_the_checker():
    for v in (0.0, 0.25, -0.5, 1.5, 3.0000000001, -1234.56789, 32768.0):
        assert stream.delay_word(v) == pc.delay_word(v)
    for v in (0.0, 20.0, -40.0, 244.0):
        assert stream.sfo_word(v) == pc.sfo_word(v)


@pytest.mark.parametrize("shift", [0, 1, 7, -3, 40])
def test_whole_sample_delay_is_a_copy(shift):
    x = rows(2, 50, 1)
    y = pc.propagate_host(x, delay=shift << 32)
    want = np.zeros_like(x)
    if shift >= 0:
        want[:, shift:] = x[:, :50 - shift]
    else:
        want[:, :50 + shift] = x[:, -shift:]
    assert np.array_equal(bits(y), bits(want))


def test_splits_and_windows_equal_the_whole():
    x = rows(2, 300, 2)
    kw = dict(delay=[[pc.delay_word(2.3), pc.delay_word(-1.75), 5 << 32]], gain=[[1.0, 0.5j, -0.25 + 0.1j]],
              sfo=[1 << 20, -(1 << 19)], fcw=[123456789 << 32, -(7 << 40)], rate=[1 << 44, -(3 << 41)],
              phase=[1 << 30, -5])
    whole = pc.propagate_host(x, 320, first_sample=1000, in_first=1003, **kw)
    assert np.count_nonzero(whole) > 500
    for cut in (1, 128, 319):
        a = pc.propagate_host(x, cut, first_sample=1000, in_first=1003, **kw)
        b = pc.propagate_host(x, 320 - cut, first_sample=1000 + cut, in_first=1003, **kw)
        assert np.array_equal(bits(np.concatenate([a, b], axis=1)), bits(whole))
    # outputs 100..199 read recording samples 1000 + 100 - 5 - 8 - 1 .. 1000 + 199 + 2 + 8 + 1 at the most
    lo, hi = 1086 - 1003, 1211 - 1003
    part = pc.propagate_host(x[:, lo:hi], 100, first_sample=1100, in_first=1003 + lo, **kw)
    assert np.array_equal(bits(part), bits(whole[:, 100:200]))


def test_rotation_without_rate_is_the_impairment_stages():
    x = rows(2, 200, 3)
    fcw32, ph = [123456789, -(1 << 31)], [-77, 1 << 29]
    first = (1 << 33) + 5
    want = ic.impair_host(x, fcw=fcw32, phase=ph, first_sample=first)
    got = pc.propagate_host(x, delay=0, fcw=[f << 32 for f in fcw32], phase=ph, first_sample=first, in_first=first)
    assert np.array_equal(bits(got), bits(want))
    # fcw alone and phase alone
    assert np.array_equal(bits(pc.propagate_host(x, fcw=[f << 32 for f in fcw32])), bits(ic.impair_host(x, fcw=fcw32)))
    assert np.array_equal(bits(pc.propagate_host(x, phase=ph)), bits(ic.impair_host(x, phase=ph)))


def test_triangle_number_modulo_2_64():
    ns = [0, 1, 2, 3, (1 << 32) - 1, 1 << 32, (1 << 33) + 5, (1 << 40) - 1, 1 << 40]
    got = pc.tri(np.array(ns, np.uint64))
    for n, g in zip(ns, got.tolist()):
        assert g == (n * (n - 1) // 2) % (1 << 64), n
    n = (1 << 40) - 1
    assert n * (n - 1) // 2 > 1 << 64      # the product itself does not fit: the modulus matters
    # the word at the far end, against Python integers
    fcw, rate, ph = -(5 << 40) + 12345, (3 << 30) + 1, -9
    W = (((ph & 0xFFFFFFFF) << 32) + (fcw % (1 << 64)) * n + (rate % (1 << 64)) * (n * (n - 1) // 2)) % (1 << 64)
    top = W >> 32
    top -= (1 << 32) if top >= 1 << 31 else 0
    want = np.float32(top) * ic.K
    got = pc.rotation_angle(np.array([n], np.uint64), fcw, rate, ph)
    assert got.dtype == np.float32 and got[0] == want
