"""GPU: both down-converter banks reading raw SDR samples (cs16, cs8, cu8 - int16, int8 and uint8
[.., 2] tensors given to stream.Channelizer.run; lora_channelize_raw_batch and
lora_resample_channelize_raw_batch), compared as fp32 bit patterns with the banks' host models
(tests/channel_checker.py, tests/resample_checker.py) applied to the conversion's host model
(tests/raw_checker.py, to_cf32), and with the float path on stream.raw_to_complex of the same
tensor: an identity with no tolerance.

The kernels load two samples at a time on the grid of that size - 8 bytes of cs16, 4 of an 8-bit
format - and load singly the sample that hangs over either end of a tile's samples.  The
alignment cases are set wider than that: they walk a row's first sample over every position of a
16-byte line (4 cs16 or 8 8-bit samples, `per_vector` below) and the row lengths around that
size, which covers the pair grid and any wider load a later kernel may use.  Inputs are uniform
over each format's whole range with the extreme codes and 0 forced in."""
import functools

import numpy as np
import pytest

from tests import channel_checker as cc
from tests import raw_checker as rk
from tests import resample_checker as rc
from tests.test_gpu_channelize import SHAPES as INTEGER_SHAPES
from tests.test_gpu_channelize import assert_same_bits, cbits, taps_of
from tests.test_gpu_resample import SHAPES as RATIONAL_SHAPES

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FORMATS = {"cs16": np.int16, "cs8": np.int8, "cu8": np.uint8}
PER_VECTOR = {"cs16": 4, "cs8": 8, "cu8": 8}
fmt_param = pytest.mark.parametrize("fmt", sorted(FORMATS))


@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import lora_phy_amd

    return lora_phy_amd


def raw_noise(fmt, shape, seed) -> np.ndarray:
    """[*shape, 2] codes uniform over the format's range; the lowest and the highest code, and 0
    where there are three components or more, are written over the first, last and middle one."""
    nd = FORMATS[fmt]
    info = np.iinfo(nd)
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    a = np.random.default_rng(seed).integers(info.min, info.max + 1, shape + (2,)).astype(nd)
    flat = a.reshape(-1)
    if flat.size >= 2:
        flat[0], flat[-1] = info.min, info.max
    if flat.size >= 3:
        flat[flat.size // 2] = 0
    return a


def host(raw, h, steps, period, D, Li=1, first=0, scale=None):
    x = rk.to_cf32(raw, scale)
    if Li == 1:
        return cc.channelize_host(x, h, steps, period, D, first)
    return rc.resample_host(x, h, steps, period, Li, D, first)


def outputs(L, T, D, Li=1):
    return cc.outputs(L, T, D) if Li == 1 else rc.outputs(L, T, Li, D)


def assert_same_bits_but_nan(got, want):
    """Every element that is not NaN has the same bits, and the NaNs are in the same places (a
    NaN's sign and payload are the processor's choice: include/lora_mi355x.h)."""
    assert got.shape == want.shape
    g, w = cbits(got), cbits(want)
    gn = np.isnan(np.stack([got.real, got.imag], -1))
    wn = np.isnan(np.stack([want.real, want.imag], -1))
    assert np.array_equal(gn, wn)
    assert np.array_equal(g[~wn], w[~wn])


# ---- 1. the banks' own shapes ----------------------------------------------------------------

@fmt_param
@pytest.mark.parametrize("T,D,period,steps,L,tile", INTEGER_SHAPES)
def test_integer_bank_equals_the_host_model_bit_for_bit(amd, fmt, T, D, period, steps, L, tile):
    raw, h = raw_noise(fmt, L, 300 + T + L), taps_of(T, T)
    chan = amd.stream.Channelizer(D, h, period, steps)
    got = chan.run(torch.from_numpy(raw).cuda())
    torch.cuda.synchronize()
    assert got.shape == (len(steps), cc.outputs(L, T, D)) and got.dtype == torch.complex64
    assert_same_bits(got.cpu().numpy(), host(raw, h, steps, period, D))


@fmt_param
@pytest.mark.parametrize("T,Li,D,period,steps,L,tile,cg,waves", RATIONAL_SHAPES)
def test_rational_bank_equals_the_host_model_bit_for_bit(amd, fmt, T, Li, D, period, steps, L, tile, cg, waves):
    raw, h = raw_noise(fmt, L, 300 + T + L), taps_of(T, T)
    chan = amd.stream.Channelizer(D, h, period, steps, interp=Li)
    got = chan.run(torch.from_numpy(raw).cuda())
    torch.cuda.synchronize()
    assert got.shape == (len(steps), rc.outputs(L, T, Li, D)) and got.dtype == torch.complex64
    assert_same_bits(got.cpu().numpy(), host(raw, h, steps, period, D, Li))


# ---- 2. every position of a row's first sample in a 16-byte vector ---------------------------

@fmt_param
@pytest.mark.parametrize("T,Li,D", [(1, 1, 1), (1, 1, 3), (7, 1, 1), (7, 1, 3), (7, 2, 3)])
def test_every_base_offset_and_row_lengths_around_a_vector(amd, fmt, T, Li, D):
    pv = PER_VECTOR[fmt]
    period, steps = 5, (1, -2)
    h = taps_of(T, 20 + T)
    chan = amd.stream.Channelizer(D, h, period, steps, interp=Li)
    lengths = [L for L in sorted({T, pv - 1, pv, pv + 1, 2 * pv + 3}) if outputs(L, T, D, Li) > 0]
    assert len(lengths) >= 2 and lengths[-1] == 2 * pv + 3
    base = raw_noise(fmt, 8 + max(lengths), 50 + T + D)
    dev = torch.from_numpy(base).cuda()
    assert dev.data_ptr() % 16 == 0
    for k in range(8):
        for L in lengths:
            part = dev[k:k + L]
            assert part.data_ptr() == dev.data_ptr() + 2 * k * base.itemsize
            got = chan.run(part).cpu().numpy()
            assert_same_bits(got, host(base[k:k + L], h, steps, period, D, Li))
        # raw[k:] of the allocation: the tail of the row is not a whole vector either
        got = chan.run(dev[k:], first_sample=k).cpu().numpy()
        assert_same_bits(got, host(base[k:], h, steps, period, D, Li, first=k))


# ---- 3. rows at three offsets within a 16-byte line ------------------------------------------

@fmt_param
@pytest.mark.parametrize("T,Li,D", [(65, 1, 8), (41, 2, 5)])
def test_rows_an_odd_number_of_samples_apart(amd, fmt, T, Li, D):
    period, steps, R = 5, (-2, 1, 2), 3
    L = T + D * 70
    stride = L + 5 + (L % 2)  # odd: the rows start at three different offsets within a 16-byte line
    assert stride % 2 == 1
    h = taps_of(T, 77)
    base = raw_noise(fmt, (R, stride), 78)
    dev = torch.from_numpy(base).cuda()
    starts = {(dev[r].data_ptr() % 16) for r in range(R)}
    assert len(starts) == 3
    chan = amd.stream.Channelizer(D, h, period, steps, interp=Li)
    want = host(base[:, :L], h, steps, period, D, Li)
    W = outputs(L, T, D, Li)
    assert want.shape == (R, len(steps), W) and W > 64
    view = dev[:, :L]
    assert not view.is_contiguous()
    got = chan.run(view)
    assert got.shape == (R, len(steps), W)
    assert_same_bits(got.cpu().numpy(), want)
    assert_same_bits(chan.run(view.contiguous()).cpu().numpy(), want)
    assert_same_bits(chan.run(dev[1, :L]).cpu().numpy(), want[1])


# ---- 4. identity with the float path ---------------------------------------------------------

@fmt_param
@pytest.mark.parametrize("T,Li,D", [(33, 1, 4), (49, 3, 8)])
def test_raw_run_equals_the_float_run_on_raw_to_complex(amd, fmt, T, Li, D):
    period, steps, L = 7, (-3, 1, 2), 700
    h = taps_of(T, 5)
    raw = raw_noise(fmt, L, 6)
    dev = torch.from_numpy(raw).cuda()
    chan = amd.stream.Channelizer(D, h, period, steps, interp=Li)
    for scale in (None, 0.37, -1.0, float("inf")):
        x = amd.stream.raw_to_complex(dev, scale)
        assert x.dtype == torch.complex64 and x.shape == (L,) and x.is_cuda
        # the torch statement of the conversion is the host model's, bit for bit
        assert_same_bits_but_nan(x.cpu().numpy(), rk.to_cf32(raw, scale))
        got = chan.run(dev, scale=scale).cpu().numpy()
        want = chan.run(x).cpu().numpy()
        assert_same_bits_but_nan(got, want)
        if scale is None or np.isfinite(scale):
            assert not np.isnan(want.real).any()
            assert_same_bits(got, want)
            assert_same_bits(got, host(raw, h, steps, period, D, Li, scale=scale))
        else:
            assert np.isinf(want.real).any() or np.isnan(want.real).any()
    assert_same_bits(chan.run(dev, scale=None).cpu().numpy(),
                     chan.run(dev, scale=amd.stream.raw_scale(dev.dtype)).cpu().numpy())


# ---- 5. out= and first_sample ----------------------------------------------------------------

@fmt_param
@pytest.mark.parametrize("T,Li,D", [(33, 1, 4), (49, 3, 8)])
def test_a_wider_out_and_two_chunks(amd, fmt, T, Li, D):
    period, steps, L = 7, (-3, 1, 2), 900
    h = taps_of(T, 8)
    raw = raw_noise(fmt, L, 9)
    dev = torch.from_numpy(raw).cuda()
    chan = amd.stream.Channelizer(D, h, period, steps, interp=Li)
    want = host(raw, h, steps, period, D, Li)
    W = want.shape[1]
    sentinel = np.complex64(complex(-123.5, 321.25))
    out = torch.full((3, W + 9), complex(sentinel), dtype=torch.complex64, device="cuda")
    view = chan.run(dev, out=out)
    assert view.shape == (3, W) and view.data_ptr() == out.data_ptr()
    o = out.cpu().numpy()
    assert_same_bits(o[:, :W], want)
    assert (o[:, W:] == sentinel).all()
    # the header's chunk rule, on raw samples
    if Li == 1:
        t1 = 100
        n0, short = t1 * D, (t1 - 1) * D + T  # the second chunk overlaps the first by T - D samples
    else:
        n0 = D * 30  # n0 * interp is a multiple of decim
        t1 = n0 * Li // D
        short = -(-((t1 - 1) * D + T - 1) // Li) + 1  # the shortest predecessor that holds t1 outputs
    first = chan.run(dev[:short]).cpu().numpy()
    second = chan.run(dev[n0:], first_sample=n0).cpu().numpy()
    assert first.shape[1] == t1 and first.shape[1] + second.shape[1] == W
    assert_same_bits(np.concatenate([first, second], axis=1), want)


# ---- 6. graph capture ------------------------------------------------------------------------

@fmt_param
@pytest.mark.parametrize("T,Li,D", [(65, 1, 8), (41, 2, 5)])
def test_one_run_captured_in_a_graph_replays_the_eager_bits(amd, fmt, T, Li, D):
    period, steps, L = 5, (-2, 1, 2), T + D * 200
    h = taps_of(T, 31)
    dev = torch.from_numpy(raw_noise(fmt, L, 32)).cuda()
    chan = amd.stream.Channelizer(D, h, period, steps, interp=Li)
    eager = chan.run(dev).cpu().numpy()
    out = torch.zeros(eager.shape, dtype=torch.complex64, device="cuda")
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        chan.run(dev, out=out)  # warm the stream-side state before capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    out.zero_()
    with torch.cuda.graph(g):  # the one kernel: no parallel branches
        chan.run(dev, out=out)
    g.replay()
    torch.cuda.synchronize()
    assert_same_bits(out.cpu().numpy(), eager)


# ---- 7. end to end ---------------------------------------------------------------------------

# (sf, osr, interp, decim, period, ntaps, cutoff, scan_checker.TABLE rows, steps): three SF7
# channels, each at 0.2 <= 0.9 / 3 of full scale so that their sum does not clip (the band-limited
# interpolation overshoots at the frames' edges: at 0.25 the 5/96 signal's peak is 1.002)
E2E = {"integer": (7, 1, 1, 8, 5, 65, 0.1, (0, 2, 3), (-1, 0, 2)),
       "rational": (7, 1, 5, 96, 12, 385, None, (2, 3, 3), (-2, 0, 3))}  # 5/96: TABLE's shortest SF7 rows
AMP, SEED0 = 0.2, 7000


@functools.lru_cache(maxsize=None)
def e2e_case(kind, fmt):
    """(raw [L, 2], taps, expected channel list, expected starts, expected symbols): the existing
    wideband tests' planted signal (channel_checker.wideband, resample_checker.wideband), without
    noise, quantised by iq_io.quantize at the default scale."""
    from lora_phy_amd import iq_io
    from oracle.pyoracle import Oracle

    sf, osr, Li, D, period, T, cutoff, rows, steps = E2E[kind]
    amps = (AMP,) * len(rows)
    assert AMP <= 0.9 / len(rows) and (T - 1) % (2 * D) == 0
    if Li == 1:
        x, planted = cc.wideband(Oracle(), rows, steps, amps, D, period, cc.LEAD, cc.PAD, SEED0, 0.0)
        taps = cc.lowpass_taps(T, cutoff)
    else:
        x, planted = rc.wideband(Oracle(), rows, steps, amps, Li, D, period, rc.LEAD, rc.PAD, SEED0, 0.0)
        taps = rc.lowpass_taps(T, 0.5 / D, gain=Li)
    assert np.abs(x.real).max() < 1.0 and np.abs(x.imag).max() < 1.0  # nothing clips
    td = {"cs16": torch.int16, "cs8": torch.int8, "cu8": torch.uint8}[fmt]
    raw = iq_io.quantize(torch.from_numpy(x), td).numpy()
    shift = (T - 1) // (2 * D)
    channel = np.concatenate([np.full(len(s), c, np.int64) for c, (s, _) in enumerate(planted)])
    starts = np.concatenate([s - shift for s, _ in planted])
    syms = np.concatenate([y for _, y in planted])
    return raw, taps, channel, starts, syms


@pytest.mark.parametrize("fmt", ["cs16", "cu8"])
@pytest.mark.parametrize("kind", sorted(E2E))
def test_receive_wideband_on_raw_samples(amd, kind, fmt):
    """receive_wideband on the raw capture equals receive_wideband on raw_to_complex of it in
    every field - no tolerance - and both recover the planted frames (which the host model alone
    does too: tests/test_raw_checker.py)."""
    sf, osr, Li, D, period, T, cutoff, rows, steps = E2E[kind]
    raw, taps, channel, starts, syms = e2e_case(kind, fmt)
    S = syms.shape[1]
    plan = amd.DemodPlan(sf, osr, dechirp=True)
    chan = amd.stream.Channelizer(D, taps, period, steps, interp=Li)
    dev = torch.from_numpy(raw).cuda()
    a_ch, a_st, a = amd.stream.receive_wideband(plan, chan, dev, S)
    b_ch, b_st, b = amd.stream.receive_wideband(plan, chan, amd.stream.raw_to_complex(dev), S)
    torch.cuda.synchronize()
    assert a_ch.dtype == a_st.dtype == torch.int64 and a_ch.is_cuda and a_st.is_cuda
    assert torch.equal(a_ch, b_ch) and torch.equal(a_st, b_st)
    assert torch.equal(a.symbols, b.symbols) and torch.equal(a.sync, b.sync)
    for name in ("cfo", "time_offset", "max_amp"):
        ga, gb = getattr(a, name).cpu().numpy(), getattr(b, name).cpu().numpy()
        assert ga.dtype == np.float32 and np.array_equal(ga.view(np.uint32), gb.view(np.uint32)), name
    # the planted truth: the channel, the start to the finder's resolution (osr samples), the symbols
    assert a_ch.cpu().tolist() == channel.tolist()
    assert a_st.shape == starts.shape and (np.abs(a_st.cpu().numpy() - starts) <= osr).all()
    assert np.array_equal(a.symbols.cpu().numpy() % (1 << sf), syms)
    assert (a.sync.cpu().numpy() == 0x12).all()
    # an explicit scale goes through: twice the scale is twice the amplitude, the same frames
    c_ch, c_st, c = amd.stream.receive_wideband(plan, chan, dev, S, scale=2 * amd.stream.raw_scale(dev.dtype))
    assert torch.equal(c_ch, a_ch) and torch.equal(c_st, a_st) and torch.equal(c.symbols, a.symbols)
    assert np.array_equal(c.max_amp.cpu().numpy(), 2 * a.max_amp.cpu().numpy())


def test_work_wideband_takes_raw_samples(amd):
    kind, fmt = "integer", "cu8"
    sf, osr, Li, D, period, T, cutoff, rows, steps = E2E[kind]
    raw, taps, channel, starts, syms = e2e_case(kind, fmt)
    demod = amd.LoRaDemod(sf, mtu=4, osr=osr)
    chan = amd.stream.Channelizer(D, taps, period, steps)
    got_ch, got_st, got = demod.work_wideband(chan, torch.from_numpy(raw).cuda(), syms.shape[1])
    torch.cuda.synchronize()
    assert got_ch.cpu().tolist() == channel.tolist() and (np.abs(got_st.cpu().numpy() - starts) <= osr).all()
    assert got.shape == (len(starts), 4) and np.array_equal(got.cpu().numpy() % (1 << sf), syms[:, :4])
    assert demod.sync_ok().all()
    got2 = demod.work_wideband(chan, torch.from_numpy(raw).cuda(), syms.shape[1], scale=0.5)
    assert got2[0].cpu().tolist() == channel.tolist()


# ---- 8. what the Python layer refuses before any launch --------------------------------------

def test_bad_raw_tensors_are_refused(amd):
    chan = amd.stream.Channelizer(3, taps_of(7, 1), 5, (1, -1))
    good = torch.zeros((40, 2), dtype=torch.int16, device="cuda")
    assert chan.run(good).shape == (2, 12)
    for bad in (torch.zeros(40, dtype=torch.int16, device="cuda"),            # [L]
                torch.zeros((40, 3), dtype=torch.int16, device="cuda"),       # [L, 3]
                torch.zeros((40, 4), dtype=torch.uint8, device="cuda")[:, ::2],   # a non-unit last stride
                torch.zeros((80, 2), dtype=torch.int8, device="cuda")[::2],   # sample stride 4
                torch.zeros((2, 41, 2), dtype=torch.int8, device="cuda").transpose(0, 1),
                torch.zeros((2, 2, 40, 2), dtype=torch.int8, device="cuda")):
        with pytest.raises(ValueError):
            chan.run(bad)
    rows = torch.zeros((3, 50, 2), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        chan.run(rows.as_strided((3, 40, 2), (61, 2, 1)))     # rows an odd number of elements apart
    with pytest.raises(ValueError):
        chan.run(rows.as_strided((3, 40, 2), (60, 2, 1)))     # overlapping rows
    for dtype in (torch.int32, torch.int64, torch.bool):
        with pytest.raises(TypeError):
            chan.run(torch.zeros((40, 2), dtype=dtype, device="cuda"))
    with pytest.raises(TypeError):
        chan.run(torch.zeros((40, 2), dtype=torch.int16))     # a CPU tensor: no CPU fallback
    with pytest.raises(TypeError):
        chan.run(torch.zeros((40, 2), dtype=torch.float32, device="cuda"))   # as before: not complex64
    with pytest.raises(ValueError):
        chan.run(torch.zeros(40, dtype=torch.complex64, device="cuda"), scale=1.0)
    with pytest.raises(ValueError):
        chan.run(good, first_sample=-1)
    plan = amd.DemodPlan(7, dechirp=True)
    with pytest.raises(ValueError):
        amd.stream.receive_wideband(plan, chan, torch.zeros((2, 4000, 2), dtype=torch.int8, device="cuda"), 6)
    with pytest.raises(ValueError):
        amd.stream.receive_wideband(plan, chan, torch.zeros(4000, dtype=torch.int8, device="cuda"), 6)
    # an empty stream and rows too short for one output: empty results, no launch
    assert chan.run(good[:0]).shape == (2, 0) and chan.run(good[:6]).shape == (2, 0)
    assert chan.run(torch.zeros((3, 2, 2), dtype=torch.uint8, device="cuda")).shape == (3, 2, 0)
