"""GPU: the rational-rate down-converter bank (stream.Channelizer with interp > 1,
lora_resample_channelize_batch) against the numpy restatement of its definition
(tests/resample_checker.py), compared as fp32 bit patterns, and the wideband receive chain built
on it against frames planted in a wideband signal at decim / interp times the channel rate.

The kernel's geometry (csrc/lora_resample.hip, resample_geometry): with reach = max over the
residues r of off[r] + K[r], a channel takes entries(tile) = decim * (tile + (reach-1) // decim)
LDS entries; a workgroup makes the outputs of 64 consecutive u of every channel where channels *
entries(64) <= 8192, else 32, 16 or 8; at 8 the channels are taken in passes of as many as fit.
A wavefront takes one residue of a group of 2 * 64 / tile channels at a time, and the workgroup
has the fewest wavefronts of 4 .. 8 with which the interp * ceil(channels per pass / group) items
take the fewest rounds.  The shapes below reach each of those paths."""
import functools

import numpy as np
import pytest

from tests import channel_checker as cc
from tests import resample_checker as rc
from tests.test_gpu_channelize import SHAPES as INTEGER_SHAPES
from tests.test_gpu_channelize import assert_same_bits, cbits, noise, special_rows, taps_of

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import lora_phy_amd

    return lora_phy_amd


def geometry_of(T, Li, D, C):
    """resample_geometry's (tile, channels per pass, wavefronts), restated."""
    reach = rc.reach(T, Li, D)

    def entries(tile):
        return D * (tile + (reach - 1) // D)

    tile = 64
    while tile > 8 and C * entries(tile) > 8192:
        tile //= 2
    cg = min(C, 8192 // entries(tile))
    items = Li * -(-cg // (2 * (64 // tile)))
    waves = min(range(4, 9), key=lambda w: (-(-items // w), w))
    return tile, cg, waves


# (ntaps, interp, decim, period, steps, L, the tile the kernel takes, channels per pass, wavefronts)
SHAPES = [
    (1, 1, 1, 1, (0,), 17, 64, 1, 4),                                          # a scaled copy
    (2, 3, 4, 5, (1, -1), 40, 64, 2, 4),                                       # a residue with no tap: exact +0.0
    (5, 2, 3, 5, (0, 2), 3, 64, 2, 4),                                         # W = 1
    (41, 2, 5, 5, (-2, -1, 0, 1, 2), 5 * 150 + 41, 64, 5, 6),                  # K differs by residue; tiles and a part
    (49, 3, 8, 16, (-4, 5), 8 * 130 + 49, 64, 2, 4),
    (7, 3, 3, 4, (1,), 100, 64, 1, 4),                                         # interp = decim
    (9, 4, 6, 7, (3,), 200, 64, 1, 4),                                         # gcd(interp, decim) > 1
    (385, 5, 96, 12, tuple(range(-4, 4)), 96 * 140 + 385, 8, 8, 5),            # tile 8, all channels in one pass
    (4096, 16, 256, 4096, tuple(range(-16, 16)), 256 * 20 + 4096, 8, 3, 8),    # the extreme: 11 passes of 3
    (49, 3, 8, 16, tuple(range(-8, 8)), 8 * 130 + 49, 32, 16, 6),              # tile 32
    (385, 5, 96, 12, (-3, -1, 1, 3), 96 * 60 + 385, 16, 4, 5),                 # tile 16
    (97, 3, 8, 16, tuple(range(-16, 16)), 8 * 100 + 97, 16, 32, 6),            # tile 16, 32 channels
    (300, 7, 9, 9, tuple(range(9)), 9 * 700, 64, 9, 7),                        # more residues than wavefronts
]


@pytest.mark.parametrize("T,Li,D,period,steps,L,tile,cg,waves", SHAPES)
def test_outputs_equal_the_host_model_bit_for_bit(amd, T, Li, D, period, steps, L, tile, cg, waves):
    assert geometry_of(T, Li, D, len(steps)) == (tile, cg, waves)
    x, h = noise(L, 100 + T + L), taps_of(T, T)
    chan = amd.stream.Channelizer(D, h, period, steps, interp=Li)
    W = rc.outputs(L, T, Li, D)
    assert W > 0 and chan.outputs(L) == W and chan.delay == (T - 1) / (2 * Li)
    got = chan.run(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    assert got.shape == (len(steps), W) and got.dtype == torch.complex64
    want = rc.resample_host(x, h, steps, period, Li, D)
    assert_same_bits(got.cpu().numpy(), want)
    if (T, Li, D) == (2, 3, 4):
        assert (cbits(got.cpu().numpy()[:, 1::3]) == 0).all()  # the residue with no tap: +0.0f
    if L == 3:
        assert W == 1


def run_c_entry(amd, entry, x, h, steps, period, D, interp=None):
    """Call lora_channelize_batch (interp None) or lora_resample_channelize_batch directly."""
    from lora_phy_amd import _capi

    lib = _capi.lib()
    xd, hd = torch.from_numpy(x).cuda(), torch.from_numpy(h).cuda()
    w = torch.from_numpy(amd.stream.nco_table(period)).cuda()
    st = (_capi.C.c_int32 * len(steps))(*steps)
    L, T = len(x), len(h)
    W = cc.outputs(L, T, D)
    out = torch.zeros((len(steps), W), dtype=torch.complex64, device="cuda")
    rates = (T, D) if interp is None else (T, interp, D)
    got = getattr(lib, entry)(xd.data_ptr(), 1, L, L, 0, hd.data_ptr(), *rates, w.data_ptr(), period, st, len(steps),
                              out.data_ptr(), W, torch.cuda.current_device(),
                              torch.cuda.current_stream().cuda_stream)
    assert got == W, (got, _capi.lib().lora_last_error())
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("T,D,period,steps,L", [INTEGER_SHAPES[3][:5], INTEGER_SHAPES[6][:5]])
def test_interp_one_through_the_new_entry_equals_the_integer_bank(amd, T, D, period, steps, L):
    x, h = noise(L, 100 + T + L), taps_of(T, T)
    new = run_c_entry(amd, "lora_resample_channelize_batch", x, h, steps, period, D, interp=1)
    old = run_c_entry(amd, "lora_channelize_batch", x, h, steps, period, D)
    assert old.shape[1] > 64
    assert_same_bits(new, old)


def test_row_lengths_around_one_output(amd):
    T, Li, D, period, steps = 7, 2, 3, 5, (1, -1)
    h = taps_of(T, 9)
    chan = amd.stream.Channelizer(D, h, period, steps, interp=Li)
    # span = 2 L - 1: one output from span 7 (L = 4), two from span 10 (L = 6: span 11)
    for L, W in ((3, 0), (4, 1), (5, 1), (6, 2)):
        x = noise(L, L)
        got = chan.run(torch.from_numpy(x).cuda())
        assert got.shape == (2, W) and chan.outputs(L) == W == rc.outputs(L, T, Li, D)
        assert_same_bits(got.cpu().numpy(), rc.resample_host(x, h, steps, period, Li, D))
    # no output: an empty tensor and no launch, for an empty stream too
    assert chan.run(torch.zeros(0, dtype=torch.complex64, device="cuda")).shape == (2, 0)
    assert chan.run(torch.zeros((3, 2), dtype=torch.complex64, device="cuda")).shape == (3, 2, 0)


def test_first_sample_needs_64_bit_arithmetic(amd):
    T, Li, D, period, steps, L = 7, 2, 3, 4093, (1, -1, 2046), 200
    first = 2 ** 40 + 3
    x, h = noise(L, 40), taps_of(T, 40)
    chan = amd.stream.Channelizer(D, h, period, steps, interp=Li)
    got = chan.run(torch.from_numpy(x).cuda(), first_sample=first).cpu().numpy()
    assert_same_bits(got, rc.resample_host(x, h, steps, period, Li, D, first))
    assert not np.array_equal(got, rc.resample_host(x, h, steps, period, Li, D, 0))
    with pytest.raises(ValueError):
        chan.run(torch.from_numpy(x).cuda(), first_sample=-1)


def test_two_chunks_equal_the_whole_run(amd):
    T, Li, D, period, steps = 49, 3, 8, 7, (-3, 1, 2)
    x, h = noise(900, 5), rc.lowpass_taps(T, 0.5 / D, gain=Li)
    chan = amd.stream.Channelizer(D, h, period, steps, interp=Li)
    xd = torch.from_numpy(x).cuda()
    whole = chan.run(xd).cpu().numpy()
    n0 = 8 * 30  # n0 * interp is a multiple of decim: 90 outputs come before it
    t1 = n0 * Li // D
    short = -(-((t1 - 1) * D + T - 1) // Li) + 1  # the shortest predecessor that holds them
    first = chan.run(xd[:short]).cpu().numpy()
    second = chan.run(xd[n0:], first_sample=n0).cpu().numpy()
    assert first.shape[1] == t1 and first.shape[1] + second.shape[1] == whole.shape[1]
    assert_same_bits(np.concatenate([first, second], axis=1), whole)
    assert_same_bits(whole, rc.resample_host(x, h, steps, period, Li, D))
    odd = chan.run(xd[n0 + 1:], first_sample=n0 + 1).cpu().numpy()  # starts off the 16-byte grid
    assert_same_bits(odd, rc.resample_host(x[n0 + 1:], h, steps, period, Li, D, n0 + 1))


def test_rows_strided_rows_and_a_wider_out(amd):
    T, Li, D, period, steps, L = 41, 2, 5, 5, (-2, 1, 2), 41 + 5 * 70
    h = taps_of(T, 77)
    x = noise((3, L), 78)
    chan = amd.stream.Channelizer(D, h, period, steps, interp=Li)
    want = rc.resample_host(x, h, steps, period, Li, D)
    W = rc.outputs(L, T, Li, D)
    assert want.shape == (3, 3, W) and W > 128
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
    with pytest.raises(TypeError):
        chan.run(torch.from_numpy(x))  # no CPU fallback


def test_nan_inf_and_negative_zero(amd):
    """The integer bank's special rows (tests/test_gpu_channelize.py, special_rows), through
    interp 2, decim 3 with 13 taps: 7 or 6 per output, so an output's window is the 7 samples that
    test's is.  Row 0 holds NaN, infinities and -0.0 where IEEE 754 fixes every bit of every
    result, and must equal the checker bit for bit.  In row 1 the NaNs are ones whose sign and
    payload IEEE 754 leaves to the processor: there every output that is not NaN must equal the
    checker's bits, and the NaNs must be exactly where the checker has them."""
    T, Li, D, period, steps = 13, 2, 3, 5, (1, 2)
    h = taps_of(T, 12)
    x = special_rows()
    chan = amd.stream.Channelizer(D, h, period, steps, interp=Li)
    got = chan.run(torch.from_numpy(x).cuda()).cpu().numpy()
    want = rc.resample_host(x, h, steps, period, Li, D)
    assert np.isnan(want[0].real).any() and np.isinf(want[0].real).any() and np.isinf(want[0].imag).any()
    # (a sum that starts at +0.0 never gives -0.0: windows of -0.0 samples come out as +0.0)
    assert (cbits(want[0]) == 0).any() and (cbits(want[0]) != 0x80000000).all()
    assert_same_bits(got[0], want[0])
    g, w = cbits(got[1]), cbits(want[1])
    gn, wn = np.isnan(np.stack([got[1].real, got[1].imag], -1)), np.isnan(np.stack([want[1].real, want[1].imag], -1))
    assert wn.any() and np.array_equal(gn, wn)
    assert np.array_equal(g[~wn], w[~wn])


# ---- the wideband receive chain -------------------------------------------------------------

E2E = [(ci, sigma) for ci in range(len(rc.CONFIGS)) for sigma in rc.SIGMAS]


@functools.lru_cache(maxsize=None)
def e2e_case(ci, sigma):
    """(x, taps, host channel rows, expected channel list, expected starts, expected symbols):
    what tests/test_resample_checker.py establishes that the host run recovers."""
    from oracle.pyoracle import Oracle

    sf, osr, Li, D, period, T, rows, steps, amps = rc.CONFIGS[ci]
    x, planted, taps = rc.config_signal(Oracle(), ci, sigma)
    shift = (T - 1) // (2 * D)
    channel = np.concatenate([np.full(len(s), c, np.int64) for c, (s, _) in enumerate(planted)])
    starts = np.concatenate([s - shift for s, _ in planted])
    syms = np.concatenate([y for _, y in planted])
    return x, taps, rc.resample_host(x, taps, steps, period, Li, D), channel, starts, syms


@pytest.mark.parametrize("ci,sigma", E2E)
def test_receive_wideband_returns_the_planted_frames(amd, ci, sigma):
    sf, osr, Li, D, period, T, rows, steps, amps = rc.CONFIGS[ci]
    x, taps, host_rows, channel, starts, syms = e2e_case(ci, sigma)
    S = syms.shape[1]
    plan = amd.DemodPlan(sf, osr, dechirp=True)
    chan = amd.stream.Channelizer(D, amd.stream.lowpass_taps(T, 0.5 / D, gain=Li), period, steps, interp=Li)
    assert np.array_equal(chan.taps.cpu().numpy(), taps) and chan.delay == (T - 1) / (2 * Li)
    xd = torch.from_numpy(x).cuda()
    got_ch, got_st, res = amd.stream.receive_wideband(plan, chan, xd, S)
    torch.cuda.synchronize()
    assert got_ch.dtype == got_st.dtype == torch.int64 and got_ch.is_cuda and got_st.is_cuda
    assert got_ch.cpu().tolist() == channel.tolist()
    assert got_st.cpu().tolist() == starts.tolist()
    assert np.array_equal(res.symbols.cpu().numpy() % (1 << sf), syms)
    assert (res.sync.cpu().numpy() == 0x12).all()
    assert_same_bits(chan.run(xd).cpu().numpy(), host_rows)


@pytest.mark.parametrize("ci,sigma", E2E)
def test_work_wideband_returns_the_planted_frames(amd, ci, sigma):
    sf, osr, Li, D, period, T, rows, steps, amps = rc.CONFIGS[ci]
    x, taps, _, channel, starts, syms = e2e_case(ci, sigma)
    demod = amd.LoRaDemod(sf, mtu=4, osr=osr)
    chan = amd.stream.Channelizer(D, taps, period, steps, interp=Li)
    got_ch, got_st, got = demod.work_wideband(chan, torch.from_numpy(x).cuda(), syms.shape[1])
    torch.cuda.synchronize()
    assert got_ch.cpu().tolist() == channel.tolist() and got_st.cpu().tolist() == starts.tolist()
    assert got.shape == (len(starts), 4) and np.array_equal(got.cpu().numpy(), syms[:, :4])
    assert demod.last is not None and np.array_equal(demod.last.symbols.cpu().numpy(), syms)
    assert demod.sync_ok().all()
