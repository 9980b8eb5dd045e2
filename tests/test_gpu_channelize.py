"""GPU: the down-converter bank (lora_phy_amd.stream.Channelizer, lora_channelize_batch) against
the numpy restatement of its definition (tests/channel_checker.py), compared as fp32 bit
patterns, and the wideband receive chain built on it against frames planted in a wideband
signal.

The kernel's tile (csrc/lora_bank.h, channel_geometry): a workgroup makes 64 outputs of
every channel where channels * decim * (64 + (ntaps-1) // decim) <= 8192 LDS entries, else 32,
16 or 8; at 8 the channels are taken in passes of as many as fit.  The shapes below reach each
of those paths."""
import functools

import numpy as np
import pytest

from tests import channel_checker as cc
from tests import detect_checker as dc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import lora_phy_amd

    return lora_phy_amd


@pytest.fixture(scope="module")
def O():
    from oracle.pyoracle import Oracle

    return Oracle()


def cbits(a) -> np.ndarray:
    """fp32 bit patterns of a complex64 array, [.., 2] (real, imaginary)."""
    a = np.ascontiguousarray(a, np.complex64)
    return np.stack([dc.bits(a.real), dc.bits(a.imag)], axis=-1)


def assert_same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    g, w = cbits(got), cbits(want)
    bad = np.argwhere(g != w)
    assert bad.size == 0, [(tuple(i), hex(g[tuple(i)]), hex(w[tuple(i)])) for i in bad[:8]] + [len(bad)]


def noise(shape, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


def taps_of(T, seed):
    return np.random.default_rng(seed).standard_normal(T).astype(np.float32)


def tile_of(T, D, C):
    """channel_geometry's tile, restated."""
    tile = 64
    while tile > 8 and C * D * (tile + (T - 1) // D) > 8192:
        tile //= 2
    return tile


# (ntaps, decim, period, steps, L, the tile the kernel takes)
SHAPES = [
    (1, 1, 1, (0,), 17, 64),                                    # a scaled copy
    (7, 3, 5, (-2, 0, 7), 100, 64),
    (3, 8, 4, (1,), 64, 64),                                    # ntaps < decim
    (65, 8, 5, (-2, -1, 0, 1, 2), 8 * 300 + 65, 64),            # W = 301: four tiles and a part
    (65, 8, 5, (-2, -1, 0, 1, 2), 65 + 8 * 128, 64),            # W = 129: one more than two tiles of 64
    (512, 64, 4096, (2047, -2047), 8192, 32),
    (33, 4, 64, tuple(range(-16, 16)), 33 + 4 * 70, 32),        # 32 channels
    (257, 16, 100, tuple(range(16)), 257 + 16 * 40, 16),
    (512, 64, 4096, tuple(range(-16, 16)), 512 + 64 * 20, 8),   # tile 8, the channels in 4 passes of 8
]


@pytest.mark.parametrize("T,D,period,steps,L,tile", SHAPES)
def test_outputs_equal_the_host_model_bit_for_bit(amd, T, D, period, steps, L, tile):
    assert tile_of(T, D, len(steps)) == tile
    x, h = noise(L, 100 + T + L), taps_of(T, T)
    chan = amd.stream.Channelizer(D, h, period, steps)
    assert chan.outputs(L) == cc.outputs(L, T, D) and chan.delay == (T - 1) / 2
    got = chan.run(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    assert got.shape == (len(steps), cc.outputs(L, T, D)) and got.dtype == torch.complex64
    assert_same_bits(got.cpu().numpy(), cc.channelize_host(x, h, steps, period, D))


def test_one_tap_is_a_scaled_copy(amd):
    x = noise(17, 3)
    chan = amd.stream.Channelizer(1, [0.5], 1, [0])
    assert_same_bits(chan.run(torch.from_numpy(x).cuda()).cpu().numpy()[0], (0.5 * x).astype(np.complex64))


def test_row_lengths_around_one_output(amd):
    T, D, period, steps = 7, 3, 5, (1, -1)
    h = taps_of(T, 9)
    chan = amd.stream.Channelizer(D, h, period, steps)
    for L, W in ((T - 1, 0), (T, 1), (T + D - 1, 1), (T + D, 2)):
        x = noise(L, L)
        got = chan.run(torch.from_numpy(x).cuda())
        assert got.shape == (2, W) and chan.outputs(L) == W
        assert_same_bits(got.cpu().numpy(), cc.channelize_host(x, h, steps, period, D))
    # no output: an empty tensor and no launch, for an empty stream too
    assert chan.run(torch.zeros(0, dtype=torch.complex64, device="cuda")).shape == (2, 0)
    assert chan.run(torch.zeros((3, 2), dtype=torch.complex64, device="cuda")).shape == (3, 2, 0)


def test_first_sample_needs_64_bit_arithmetic(amd):
    """k * (first_sample + n) passes 2^51 here; the oscillator index is still exact."""
    T, D, period, steps, L = 7, 3, 4093, (1, -1, 2046), 200
    first = 2 ** 40 + 3
    x, h = noise(L, 40), taps_of(T, 40)
    chan = amd.stream.Channelizer(D, h, period, steps)
    got = chan.run(torch.from_numpy(x).cuda(), first_sample=first).cpu().numpy()
    assert_same_bits(got, cc.channelize_host(x, h, steps, period, D, first))
    assert not np.array_equal(got, cc.channelize_host(x, h, steps, period, D, 0))
    with pytest.raises(ValueError):
        chan.run(torch.from_numpy(x).cuda(), first_sample=-1)


def test_two_chunks_equal_the_whole_run(amd):
    T, D, period, steps = 33, 4, 7, (-3, 1, 2)
    x, h = noise(900, 5), cc.lowpass_taps(33, 0.2)
    chan = amd.stream.Channelizer(D, h, period, steps)
    xd = torch.from_numpy(x).cuda()
    whole = chan.run(xd).cpu().numpy()
    t1 = 100
    first = chan.run(xd[:(t1 - 1) * D + T]).cpu().numpy()
    second = chan.run(xd[t1 * D:], first_sample=t1 * D).cpu().numpy()
    assert first.shape[1] == t1 and first.shape[1] + second.shape[1] == whole.shape[1]
    assert_same_bits(np.concatenate([first, second], axis=1), whole)
    assert_same_bits(whole, cc.channelize_host(x, h, steps, period, D))
    odd = chan.run(xd[(t1 * D + 1):], first_sample=t1 * D + 1).cpu().numpy()  # starts off the 16-byte grid
    assert_same_bits(odd, cc.channelize_host(x[t1 * D + 1:], h, steps, period, D, t1 * D + 1))


def test_rows_strided_rows_and_a_wider_out(amd):
    T, D, period, steps, L = 65, 8, 5, (-2, 1, 2), 65 + 8 * 70
    h = taps_of(T, 77)
    x = noise((3, L), 78)
    chan = amd.stream.Channelizer(D, h, period, steps)
    want = cc.channelize_host(x, h, steps, period, D)
    W = cc.outputs(L, T, D)
    assert want.shape == (3, 3, W)
    got = chan.run(torch.from_numpy(x).cuda())
    assert got.shape == (3, 3, W)
    assert_same_bits(got.cpu().numpy(), want)
    # a strided row view: rows L + 5 samples apart (odd rows start off the 16-byte grid)
    base = torch.full((3, L + 5), 7.0 + 7.0j, dtype=torch.complex64, device="cuda")
    base[:, :L] = torch.from_numpy(x).cuda()
    assert_same_bits(chan.run(base[:, :L]).cpu().numpy(), want)
    # out wider than W: the columns from W on are not touched
    sentinel = np.complex64(complex(-123.5, 321.25))
    out = torch.full((3, 3, W + 9), complex(sentinel), dtype=torch.complex64, device="cuda")
    view = chan.run(torch.from_numpy(x).cuda(), out=out)
    assert view.shape == (3, 3, W) and view.data_ptr() == out.data_ptr()
    o = out.cpu().numpy()
    assert_same_bits(o[..., :W], want)
    assert (o[..., W:] == sentinel).all()
    one = torch.full((3, W + 1), complex(sentinel), dtype=torch.complex64, device="cuda")
    chan.run(torch.from_numpy(x[1]).cuda(), out=one)
    assert_same_bits(one.cpu().numpy()[:, :W], want[1])
    assert (one.cpu().numpy()[:, W:] == sentinel).all()
    with pytest.raises(ValueError):
        chan.run(torch.from_numpy(x).cuda(), out=out[..., :W - 1].contiguous())
    with pytest.raises(ValueError):
        chan.run(torch.from_numpy(x).cuda(), out=out[:, :2])
    with pytest.raises(TypeError):
        chan.run(torch.from_numpy(x).cuda(), out=out.real.contiguous())
    with pytest.raises(TypeError):
        chan.run(torch.from_numpy(x))  # no CPU fallback


def special_rows():
    """Two rows of 240 samples for (ntaps 7, decim 3, period 5, steps 1 and 2).
    Row 0: NaN, +-inf and -0.0 where IEEE 754 fixes every bit of every result - an infinity meets
    no zero (no sample index that is a multiple of 5, where the table holds (1, -0)) and no second
    infinity in its window, and the NaN is the real part of its sample, which no operation
    subtracts.  Row 1: results whose NaN IEEE 754 leaves open: inf * 0, inf - inf in one product,
    +inf and -inf in one window, and a NaN imaginary part, the subtrahend of zr."""
    x = noise((2, 240), 11)
    r = x[0]
    r[3] = complex(np.inf, 0.25)
    r[41] = complex(-0.5, -np.inf)
    r[77] = complex(np.nan, 1.0)
    r[140:170] = complex(-0.0, -0.0)
    r[171] = complex(-0.0, 1.5)
    r[201] = complex(-np.inf, 3.0)
    q = x[1]
    q[5] = complex(np.inf, 1.0)       # m = 0: inf * -0
    q[33] = complex(np.inf, np.inf)   # inf - inf inside the mixing product
    q[61] = complex(np.inf, 0.0)
    q[63] = complex(-np.inf, 0.0)     # with q[61] in one window
    q[100:130] = 0
    q[173] = complex(2.0, np.nan)
    return x


def test_nan_inf_and_negative_zero(amd):
    """Row 0 must equal the checker bit for bit, its NaNs, infinities and zeros included.  In row 1
    the NaNs are ones whose sign and payload IEEE 754 leaves to the processor, as the header says:
    those born of an invalid operation, and a NaN that enters as a subtrahend (measured on the
    MI355X: (2, NaN) as a sample gives zr = 0xffc00000, the NaN's sign flipped by the
    subtraction, where x86 returns 0x7fc00000).  There every output that is not NaN must equal the
    checker's bits, and the NaNs must be exactly where the checker has them."""
    T, D, period, steps = 7, 3, 5, (1, 2)
    h = taps_of(T, 12)
    x = special_rows()
    chan = amd.stream.Channelizer(D, h, period, steps)
    got = chan.run(torch.from_numpy(x).cuda()).cpu().numpy()
    want = cc.channelize_host(x, h, steps, period, D)
    assert np.isnan(want[0].real).any() and np.isinf(want[0].real).any() and np.isinf(want[0].imag).any()
    # (a sum that starts at +0.0 never gives -0.0: windows of -0.0 samples come out as +0.0)
    assert (cbits(want[0, :, 48:54]) == 0).all() and (cbits(want[0]) != 0x80000000).all()
    assert_same_bits(got[0], want[0])
    g, w = cbits(got[1]), cbits(want[1])
    gn, wn = np.isnan(np.stack([got[1].real, got[1].imag], -1)), np.isnan(np.stack([want[1].real, want[1].imag], -1))
    assert wn.any() and np.array_equal(gn, wn)
    assert np.array_equal(g[~wn], w[~wn])


# ---- the wideband receive chain -------------------------------------------------------------

E2E = [(ci, ai, sigma) for ci in (0, 1, 4) for ai in range(len(cc.CONFIGS[ci][8])) for sigma in (0.0, 0.1)]


@functools.lru_cache(maxsize=None)
def e2e_case(ci, ai, sigma):
    """(x, taps, host channel rows, expected channel list, expected starts, expected symbols)."""
    from oracle.pyoracle import Oracle

    sf, osr, D, period, T, cutoff, rows, steps, amps = cc.CONFIGS[ci]
    x, planted, taps = cc.config_signal(Oracle(), ci, ai, sigma)
    shift = (T - 1) // 2 // D
    channel = np.concatenate([np.full(len(s), c, np.int64) for c, (s, _) in enumerate(planted)])
    starts = np.concatenate([s - shift for s, _ in planted])
    syms = np.concatenate([y for _, y in planted])
    return x, taps, cc.channelize_host(x, taps, steps, period, D), channel, starts, syms


@pytest.mark.parametrize("ci,ai,sigma", E2E)
def test_receive_wideband_returns_the_planted_frames(amd, ci, ai, sigma):
    sf, osr, D, period, T, cutoff, rows, steps, amps = cc.CONFIGS[ci]
    x, taps, host_rows, channel, starts, syms = e2e_case(ci, ai, sigma)
    S = syms.shape[1]
    plan = amd.DemodPlan(sf, osr, dechirp=True)
    chan = amd.stream.Channelizer(D, taps, period, steps)
    xd = torch.from_numpy(x).cuda()
    got_ch, got_st, res = amd.stream.receive_wideband(plan, chan, xd, S)
    torch.cuda.synchronize()
    assert got_ch.dtype == got_st.dtype == torch.int64 and got_ch.is_cuda and got_st.is_cuda
    assert got_ch.cpu().tolist() == channel.tolist()
    assert got_st.cpu().tolist() == starts.tolist()
    assert np.array_equal(res.symbols.cpu().numpy() % (1 << sf), syms)
    assert (res.sync.cpu().numpy() == 0x12).all()
    assert_same_bits(chan.run(xd).cpu().numpy(), host_rows)


def test_work_wideband_honours_mtu_and_sets_last(amd):
    ci, ai, sigma = 0, 1, 0.1
    sf, osr, D, period, T, cutoff, rows, steps, amps = cc.CONFIGS[ci]
    x, taps, _, channel, starts, syms = e2e_case(ci, ai, sigma)
    demod = amd.LoRaDemod(sf, mtu=4, osr=osr)
    chan = amd.stream.Channelizer(D, taps, period, steps)
    got_ch, got_st, got = demod.work_wideband(chan, torch.from_numpy(x).cuda(), syms.shape[1])
    torch.cuda.synchronize()
    assert got_ch.cpu().tolist() == channel.tolist() and got_st.cpu().tolist() == starts.tolist()
    assert got.shape == (len(starts), 4) and np.array_equal(got.cpu().numpy(), syms[:, :4])
    assert demod.last is not None and np.array_equal(demod.last.symbols.cpu().numpy(), syms)
    assert demod.sync_ok().all()


def test_nothing_found_makes_no_demod_call(amd):
    plan = amd.DemodPlan(7, dechirp=True)
    chan = amd.stream.Channelizer(8, cc.lowpass_taps(65, 0.1), 5, (-1, 0, 1))
    x = torch.zeros(8 * 4000, dtype=torch.complex64, device="cuda")
    for part in (x, x[:8 * 100], x[:10]):  # rows of 3992 samples, rows shorter than a window, no row at all
        ch, st, res = amd.stream.receive_wideband(plan, chan, part, 6)
        assert ch.shape == st.shape == (0,) and ch.dtype == st.dtype == torch.int64
        assert res.symbols.shape == (0, 6) and res.symbols.dtype == torch.uint16
        assert res.sync.shape == res.cfo.shape == res.time_offset.shape == res.max_amp.shape == (0,)
    assert plan.last_kernels() == set()  # run() never ran on this plan
    with pytest.raises(ValueError):
        amd.stream.receive_wideband(amd.DemodPlan(7), chan, x, 6)  # a plan that does not dechirp
    with pytest.raises(ValueError):
        amd.stream.receive_wideband(plan, chan, x, 6, hop=48)
    with pytest.raises(ValueError):
        amd.stream.receive_wideband(plan, chan, x.reshape(2, -1), 6)
    with pytest.raises(ValueError):
        amd.stream.receive_wideband(amd.DemodPlan(7, bw=250000, dechirp=True), chan, x, 6)
