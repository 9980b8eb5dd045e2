"""CPU: the numpy restatement of the channel impairment stage (tests/impair_checker.py) is the
definition in include/lora_mi355x.h: Philox4x32-10's known answers, the noise's statistics, the
invariance under chunking and row splits, the rotation against float64, and the 64-bit boundaries
of first_sample and first_row."""
import numpy as np
import pytest

from tests import impair_checker as ic

F32 = np.float32


@pytest.fixture(autouse=True, scope="module")
def the_entry_it_restates():
    """The checker is the restatement of lora_impair_batch: without that entry it checks nothing."""
    from lora_phy_amd import _capi, stream

    assert "lora_impair_batch" in _capi.EXPORTED_SYMBOLS and hasattr(_capi.lib(), "lora_impair_batch")
    for c in (0.0, 0.25 / 128, -0.3, 0.5, 1.25):
        assert stream.cfo_word(c) == ic.cfo_word(c)


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = ic.philox4x32_10(np.array(ctr, np.uint64), key)
        assert tuple(int(v) for v in got) == want
    # vectorised over the leading dimension
    both = ic.philox4x32_10(np.array([kat[0][0], kat[0][0]], np.uint64), kat[0][1])
    assert both.shape == (2, 4) and (both == np.array(kat[0][2], np.uint32)).all()


def test_counter_and_key_layout():
    """Sample n reads words (0, 1) of block n >> 1 when even and (2, 3) when odd; the counter is
    (b lo, b hi, R lo, R hi) and the key (seed lo, seed hi)."""
    seed, R = (5 << 32) | 7, (3 << 32) | 9
    n = np.array([10, 11, (1 << 33) + 4, (1 << 33) + 5], np.uint64)
    w0, w1 = ic.noise_words(seed, R, n)
    for i, b in ((0, 5), (2, (1 << 32) + 2)):
        blk = ic.philox4x32_10(np.array([b & 0xFFFFFFFF, b >> 32, 9, 3], np.uint64), (7, 5))
        assert (w0[i], w1[i], w0[i + 1], w1[i + 1]) == tuple(blk)


M = 1 << 18


@pytest.mark.parametrize("seed,row", [(2026, 0), (2026, 1), (1 << 32, 0)])
def test_noise_statistics(seed, row):
    """Every statistic within 4 standard deviations of its expectation for M independent N(0, 1)
    pairs: mean 1/sqrt(M), variance sqrt(2/M), correlations 1/sqrt(M), fourth moment sqrt(96/M)."""
    nr, ni = ic.noise(seed, row, np.arange(M, dtype=np.uint64), 1.0)
    a, b = nr.astype(np.float64), ni.astype(np.float64)
    r = 1.0 / np.sqrt(M)
    worst = 0.0
    for v in (a, b):
        stats = [(v.mean(), 0.0, r), (v.var(), 1.0, np.sqrt(2.0 / M)), ((v[1:] * v[:-1]).mean(), 0.0, r),
                 ((v ** 4).mean(), 3.0, np.sqrt(96.0 / M))]
        for got, want, sd in stats:
            worst = max(worst, abs(got - want) / sd)
    for got in ((a * b).mean(), (a[1:] * b[:-1]).mean(), (b[1:] * a[:-1]).mean()):
        worst = max(worst, abs(got) / r)
    print("worst deviation in standard deviations: %.2f" % worst)
    assert worst <= 4.0
    assert max(np.abs(a).max(), np.abs(b).max()) <= 5.77


def test_chunk_and_row_invariance():
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((3, 301)) + 1j * rng.standard_normal((3, 301))).astype(np.complex64)
    kw = dict(gain=[1.0, 0.5, 2.0], fcw=[12345678, -7, 1 << 30], phase=[0, 99, -(1 << 31)], sigma=[0.1, 0.2, 0.3],
              seed=77)
    whole = ic.impair_host(x, first_sample=1000, first_row=5, **kw)
    cut = 100
    parts = np.concatenate([ic.impair_host(x[:, :cut], first_sample=1000, first_row=5, **kw),
                            ic.impair_host(x[:, cut:], first_sample=1000 + cut, first_row=5, **kw)], axis=1)
    assert (parts.view(np.uint32) == whole.view(np.uint32)).all()
    for r in range(3):
        one = ic.impair_host(x[r], first_sample=1000, first_row=5 + r, **{k: (v[r] if isinstance(v, list) else v)
                                                                          for k, v in kw.items()})
        assert (one.view(np.uint32) == whole[r].view(np.uint32)).all()
    # noise only, and its rows
    n2 = ic.impair_host(None, 2, 64, sigma=0.5, seed=9, first_row=4)
    assert (n2[1].view(np.uint32) == ic.impair_host(None, 1, 64, sigma=0.5, seed=9, first_row=5)[0].view(np.uint32)).all()
    assert not (n2[0] == n2[1]).any()


def test_null_stages_are_not_performed():
    """A stage that is not given does nothing to the bits: -0.0 stays -0.0 (a rotation by 0 or an
    added +0.0 would make it +0.0)."""
    x = np.array([-0.0, -0.0, 1.0, -0.0], F32).view(np.complex64)
    g = ic.impair_host(x, gain=1.0)
    assert (g.view(np.uint32) == x.view(np.uint32)).all()
    r = ic.impair_host(x, fcw=0)  # -0*1 - (-0*0) = -0 - (-0) = +0
    assert (r == x).all() and r.view(np.uint32)[0] == 0 and x.view(np.uint32)[0] == 0x80000000
    z = ic.impair_host(x, sigma=0.0)
    assert (z == x).all()


def test_rotation_against_float64():
    """|y - x exp(2 pi i fcw n / 2^32)| <= |x| * B, with B derived from the formats alone
    (e = 2^-24, the relative error of one fp32 rounding):
    * theta = fl(fl(int32 p) * K).  The conversion errs by at most e relative, K = fl(pi) 2^-31 by
      at most e relative, the product by e relative; |theta| <= pi, so the angle is off by at
      most 3 pi e and the rotated sample by |x| * 3 pi e.
    * sincosf is within 1 ulp <= 2e of values of magnitude <= 1: each component moves by at most
      (|xr| + |xi|) * 2e <= sqrt(2) |x| * 2e.
    * a component is two products and a sum: (|xr c| + |xi s|) e <= sqrt(2) |x| e for the products
      and |x| e for the sum.
    A component is therefore within |x| e (3 sqrt(2) + 1) of the exact rotation by theta, the
    complex sample within sqrt(2) times that, and B = e (3 pi + 6 + sqrt(2)) = 1.005e-6."""
    e = 2.0 ** -24
    B = e * (3 * np.pi + 6 + np.sqrt(2.0))
    rng = np.random.default_rng(5)
    L = 4096
    x = (rng.standard_normal(L) + 1j * rng.standard_normal(L)).astype(np.complex64)
    worst = 0.0
    for fcw, first in ((ic.cfo_word(0.25 / 128), 0), (-123456789, 1 << 20), (1, (1 << 40) + 3), (-(1 << 31), 7)):
        y = ic.impair_host(x, fcw=fcw, first_sample=first)
        words = [((fcw % (1 << 32)) * (first + t)) % (1 << 32) for t in range(L)]
        ref = x.astype(np.complex128) * np.exp(2j * np.pi * np.array(words, np.float64) / 2.0 ** 32)
        err = np.abs(y.astype(np.complex128) - ref) / np.abs(x.astype(np.complex128))
        worst = max(worst, float(err.max()))
        assert (err <= B).all(), (fcw, first, float(err.max()), B)
    print("worst rotation error %.3g of the bound %.3g" % (worst, B))


def test_first_sample_and_first_row_word_boundaries():
    """Across n = 2^32 and 2^33 the phase word wraps (only n mod 2^32 enters the rotation) while
    the block counter's high word begins; across R = 2^32 the row's high word does."""
    x = np.ones(8, np.complex64)
    kw = dict(fcw=ic.cfo_word(0.01), phase=5, sigma=0.25, seed=11)
    for first in ((1 << 32) - 3, (1 << 33) - 3):
        y = ic.impair_host(x, first_sample=first, **kw)
        # the rotation is that of n mod 2^32
        rot = ic.impair_host(x, first_sample=first, fcw=kw["fcw"], phase=5)
        lo = ic.impair_host(x, first_sample=first % (1 << 32), fcw=kw["fcw"], phase=5)
        assert (rot.view(np.uint32) == lo.view(np.uint32)).all()
        # the noise is not: from n = 2^32 on (2^33: everywhere) it differs from that of n mod 2^32
        low = np.concatenate([ic.impair_host(x[:3], first_sample=(1 << 32) - 3, **kw),
                              ic.impair_host(x[3:], first_sample=0, **kw)])
        assert not (y[3:] == low[3:]).any() and (y[:3] == low[:3]).all() == (first < (1 << 32))
        # sample by sample across the boundary
        for t in range(8):
            one = ic.impair_host(x[t:t + 1], first_sample=first + t, **kw)
            assert one.view(np.uint32).tolist() == y[t:t + 1].view(np.uint32).tolist()
    rows = ic.impair_host(np.ones((3, 8), np.complex64), first_row=(1 << 32) - 2, **kw)
    low = ic.impair_host(np.ones((3, 8), np.complex64), first_row=((1 << 32) - 2) % (1 << 32), **kw)
    assert (rows[:2] == low[:2]).all()
    wrapped = ic.impair_host(np.ones((1, 8), np.complex64), first_row=0, **kw)  # R = 2^32 is not R = 0
    assert not (rows[2] == wrapped[0]).any()
    # seeds that differ only above bit 31
    a = ic.impair_host(None, 1, 8, sigma=1.0, seed=3)
    b = ic.impair_host(None, 1, 8, sigma=1.0, seed=3 | (1 << 32))
    assert not (a == b).any()
