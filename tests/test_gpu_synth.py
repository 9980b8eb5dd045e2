"""GPU: the synthesis bank (lora_phy_amd.stream.Synthesizer, lora_synthesize_batch and
lora_synthesize_raw_batch) against the numpy restatement of its definition
(tests/synth_checker.py), compared as bit patterns, and the wideband transmit chain built on it
looped back through the wideband receive chain.

The kernel's geometry (csrc/lora_synth.hip): a workgroup makes a tile of 1024 outputs of one row,
four per lane; it stages (1023 // interp) + P + 1 samples per channel (or one fewer) and takes the
channels in passes of as many as fit the LDS beside the taps and the tile's stored form - among
the shapes below all of them, except 512 taps at interp 1 (passes of 4).  K is P or P - 1, the last tap
step being predicated.  The shapes below reach each of those paths with more than one tile."""
import functools

import numpy as np
import pytest

from tests import channel_checker as cc
from tests import detect_checker as dc
from tests import synth_checker as sy

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TILE = 1024
NP_OF = {torch.int16: np.int16, torch.int8: np.int8, torch.uint8: np.uint8}
RAW_DTYPES = [torch.int16, torch.int8, torch.uint8]
raw_param = pytest.mark.parametrize("dtype", RAW_DTYPES, ids=["cs16", "cs8", "cu8"])


@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import lora_phy_amd

    return lora_phy_amd


def cbits(a) -> np.ndarray:
    """fp32 bit patterns of a complex64 array, [.., 2] (real, imaginary)."""
    a = np.ascontiguousarray(a, np.complex64)
    return np.stack([dc.bits(a.real), dc.bits(a.imag)], axis=-1)


def assert_same_bits(got, want, nan_free=True):
    """Equal fp32 bit patterns.  ``nan_free=False``: where the checker has a NaN the GPU must have
    one too, of any sign and payload (the header's caveat), and everything else must be equal."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    g, w = cbits(got), cbits(want)
    if not nan_free:
        gn = np.isnan(np.stack([got.real, got.imag], -1))
        wn = np.isnan(np.stack([want.real, want.imag], -1))
        assert np.array_equal(gn, wn)
        g, w = g[~wn], w[~wn]
    bad = np.argwhere(g != w)
    assert bad.size == 0, [(tuple(i), hex(g[tuple(i)]), hex(w[tuple(i)])) for i in bad[:8]] + [len(bad)]


def noise(shape, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


def taps_of(T, seed):
    return np.random.default_rng(seed).standard_normal(T).astype(np.float32)


def tile_plus_one(T, U):
    """The chan_len that gives one tile plus one channel sample's outputs (two workgroups)."""
    return sy.phases(T, U) + -(-TILE // U)


# (interp, ntaps, period, steps, gains, chan_len or None for one tile plus one sample)
SHAPES = [
    (1, 1, 1, (0,), None, 17),                                            # a scaled copy
    (1, 2, 5, (-2, 7), (1.0, -0.5), None),
    (1, 65, 4096, (2047, -2047, 4097, -5000, 1), (0.1, 1.0, -1.0, 0.0, 2.0), None),
    (1, 512, 5, (0, 1, 2, 3, 4), None, None),                             # P = 512: passes of 4 and 1
    (2, 1, 5, (1, -1), None, None),                                       # ntaps = U - 1: phase 1 has K == 0
    (2, 2, 1, (0, 3), (0.1, -0.1), None),
    (2, 3, 5, (-6,), None, None),
    (3, 2, 5, (1, 2), (-1.0, 0.0), None),                                 # ntaps = U - 1, odd W per tile
    (3, 3, 4096, (-1, 4095, 4096, 1000, -3000), None, None),
    (3, 4, 5, (2,), (0.1,), 40),
    (3, 65, 5, (0, 1), None, None),
    (8, 7, 5, (1, 2), None, None),                                        # ntaps = U - 1
    (8, 8, 5, (-2, -1, 0, 1, 2), None, None),
    (8, 9, 1, (5,), None, None),
    (8, 65, 5, (-2, -1, 0, 1, 2), (1.0, 0.1, 1.0, 0.1, 1.0), 9 + 300),    # three tiles
    (8, 512, 4096, tuple(range(-16, 16)), None, None),                    # 32 channels
    (64, 1, 5, (1,), None, 20),                                           # 63 of 64 phases have K == 0
    (64, 63, 5, (1, -1), None, None),                                     # ntaps = U - 1
    (64, 64, 4096, (2047, -2047), (-0.5, 0.1), None),
    (64, 65, 5, (3, 4), None, None),
    (64, 512, 4096, tuple(range(-16, 16)), tuple(0.1 * (c % 3 - 1) for c in range(32)), None),
    (1, 512, 4096, tuple(range(32)), None, 512 + 40),                     # 32 channels in 8 passes of 4
    (8, 96, 5, (1, -2), None, None),                                      # every phase has K == P = 12
    (8, 89, 5, (1, -2), None, None),                                      # only phase 0 has K == P
    (8, 97, 5, (1, -2), None, None),
    (2, 23, 5, (2,), None, None),
]


@functools.lru_cache(maxsize=None)
def shape_case(i):
    """(x [C, Lc], taps, the host model's output) of SHAPES[i]: computed once, shared by the
    complex64 test and the raw ones."""
    U, T, period, steps, gains, Lc = SHAPES[i]
    Lc = tile_plus_one(T, U) if Lc is None else Lc
    x, h = noise((len(steps), Lc), 100 + 7 * i), taps_of(T, 200 + i)
    want = sy.synthesize_host(x, h, U, steps, period, gains)
    want.setflags(write=False)
    return x, h, want


@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_outputs_equal_the_host_model_bit_for_bit(amd, i):
    U, T, period, steps, gains, _ = SHAPES[i]
    x, h, want = shape_case(i)
    Lc = x.shape[1]
    syn = amd.stream.Synthesizer(U, h, period, steps, gains)
    assert syn.outputs(Lc) == sy.outputs(Lc, T, U) == len(want) and syn.delay == sy.delay(T, U)
    got = syn.run(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    assert got.shape == want.shape and got.dtype == torch.complex64
    assert_same_bits(got.cpu().numpy(), want)


@raw_param
@pytest.mark.parametrize("i", [2, 7, 14, 20])
def test_raw_outputs_equal_the_store_rule_on_the_host_model(amd, i, dtype):
    """Each raw format, written at a buffer's first sample and at its second (the store is by 16
    bytes where the address allows: the two offsets put the lines' edges elsewhere), with the
    default inv_scale and with one that saturates about a tenth of the codes."""
    U, T, period, steps, gains, _ = SHAPES[i]
    x, h, want = shape_case(i)
    W = len(want)
    syn = amd.stream.Synthesizer(U, h, period, steps, gains)
    xd = torch.from_numpy(x).cuda()
    peak = float(np.abs(np.stack([want.real, want.imag])).max())
    for inv_scale in (None, 1.8 * sy.RAW[np.dtype(NP_OF[dtype])][0] / peak):
        codes = sy.store_host(want, NP_OF[dtype], inv_scale)
        got = syn.run(xd, dtype=dtype, inv_scale=inv_scale)
        assert got.shape == (W, 2) and got.dtype == dtype
        assert np.array_equal(got.cpu().numpy(), codes)
        for k in (1, 2, 3):
            buf = torch.full((W + 11, 2), 77, dtype=dtype, device="cuda")
            view = syn.run(xd, out=buf[k:], dtype=dtype, inv_scale=inv_scale)
            assert view.shape == (W, 2) and view.data_ptr() == buf[k:].data_ptr()
            b = buf.cpu().numpy()
            assert np.array_equal(b[k:k + W], codes), k
            assert (b[:k] == 77).all() and (b[k + W:] == 77).all(), k
    assert (codes == sy.RAW[np.dtype(NP_OF[dtype])][3]).any() and (codes == sy.RAW[np.dtype(NP_OF[dtype])][2]).any()


def test_one_tap_is_a_scaled_copy(amd):
    x = noise((1, 17), 3)
    syn = amd.stream.Synthesizer(1, [0.5], 1, [0])
    assert_same_bits(syn.run(torch.from_numpy(x).cuda()).cpu().numpy(), (0.5 * x[0]).astype(np.complex64))


def test_chan_len_around_the_first_output(amd):
    U, T, period, steps = 3, 7, 5, (1, -1)
    h, P = taps_of(T, 9), 3
    syn = amd.stream.Synthesizer(U, h, period, steps)
    for Lc, W in ((P - 1, 0), (P, U), (P + 1, 2 * U)):
        x = noise((2, Lc), Lc)
        got = syn.run(torch.from_numpy(x).cuda())
        assert got.shape == (W,) and syn.outputs(Lc) == W
        assert_same_bits(got.cpu().numpy(), sy.synthesize_host(x, h, U, steps, period))
    # no output: an empty tensor and no launch, for empty streams too
    assert syn.run(torch.zeros((2, 0), dtype=torch.complex64, device="cuda")).shape == (0,)
    assert syn.run(torch.zeros((3, 2, 2), dtype=torch.complex64, device="cuda")).shape == (3, 0)
    assert syn.run(torch.zeros((2, 2), dtype=torch.complex64, device="cuda"), dtype=torch.int8).shape == (0, 2)
    assert syn.run(torch.zeros((0, 2, 9), dtype=torch.complex64, device="cuda")).shape == (0, 21)


def test_first_sample_needs_64_bit_arithmetic(amd):
    """k * (first_sample + t) passes 2^51 here; the oscillator index is still exact."""
    U, T, period, steps, Lc = 3, 7, 4093, (1, -1, 2046), 400
    first = 2 ** 40 + 3
    x, h = noise((3, Lc), 40), taps_of(T, 40)
    syn = amd.stream.Synthesizer(U, h, period, steps)
    xd = torch.from_numpy(x).cuda()
    got = syn.run(xd, first_sample=first).cpu().numpy()
    assert_same_bits(got, sy.synthesize_host(x, h, U, steps, period, first_sample=first))
    assert not np.array_equal(got, sy.synthesize_host(x, h, U, steps, period))
    got = syn.run(xd, first_sample=2 ** 31).cpu().numpy()
    assert_same_bits(got, sy.synthesize_host(x, h, U, steps, period, first_sample=2 ** 31))
    with pytest.raises(ValueError):
        syn.run(xd, first_sample=-1)


def test_two_chunks_equal_the_whole_run(amd):
    U, T, period, steps, gains = 4, 33, 7, (-3, 1, 2), (1.0, 0.5, -2.0)
    x, h = noise((3, 700), 5), sy.lowpass_taps(T, 0.5 / U, U)
    P = sy.phases(T, U)
    syn = amd.stream.Synthesizer(U, h, period, steps, gains)
    xd = torch.from_numpy(x).cuda()
    whole = syn.run(xd).cpu().numpy()
    n1 = 301  # the first chunk ends inside a tile of the whole run, and off the 16-byte grid
    first = syn.run(xd[:, :n1]).cpu().numpy()
    second = syn.run(xd[:, n1 - (P - 1):], first_sample=len(first)).cpu().numpy()
    assert len(first) == (n1 - P + 1) * U and len(first) + len(second) == len(whole)
    assert_same_bits(np.concatenate([first, second]), whole)
    assert_same_bits(whole, sy.synthesize_host(x, h, U, steps, period, gains))


def test_rows_strided_streams_and_a_wider_out(amd):
    U, T, period, steps, Lc = 8, 65, 5, (-2, 1, 2), 9 + 140
    h = taps_of(T, 77)
    x = noise((3, 3, Lc), 78)
    syn = amd.stream.Synthesizer(U, h, period, steps, (1.0, -0.5, 0.1))
    want = sy.synthesize_host(x, h, U, steps, period, (1.0, -0.5, 0.1))
    W = sy.outputs(Lc, T, U)
    assert want.shape == (3, W) and W > TILE
    got = syn.run(torch.from_numpy(x).cuda())
    assert got.shape == (3, W)
    assert_same_bits(got.cpu().numpy(), want)
    # strided streams: Lc + 5 samples apart (odd streams start off the 16-byte grid)
    base = torch.full((3, 3, Lc + 5), 7.0 + 7.0j, dtype=torch.complex64, device="cuda")
    base[..., :Lc] = torch.from_numpy(x).cuda()
    assert_same_bits(syn.run(base[..., :Lc]).cpu().numpy(), want)
    # out wider than W, rows W + 9 apart: the columns from W on are not touched
    sentinel = np.complex64(complex(-123.5, 321.25))
    out = torch.full((3, W + 9), complex(sentinel), dtype=torch.complex64, device="cuda")
    view = syn.run(torch.from_numpy(x).cuda(), out=out)
    assert view.shape == (3, W) and view.data_ptr() == out.data_ptr()
    o = out.cpu().numpy()
    assert_same_bits(o[:, :W], want)
    assert (o[:, W:] == sentinel).all()
    for dtype in RAW_DTYPES:
        raw = torch.full((3, W + 3, 2), 55, dtype=dtype, device="cuda")
        view = syn.run(torch.from_numpy(x).cuda(), out=raw, dtype=dtype)
        r = raw.cpu().numpy()
        assert view.shape == (3, W, 2)
        assert np.array_equal(r[:, :W], sy.store_host(want, NP_OF[dtype])) and (r[:, W:] == 55).all()
    one = torch.full((W + 1,), complex(sentinel), dtype=torch.complex64, device="cuda")
    syn.run(torch.from_numpy(x[1]).cuda(), out=one[1:])        # an out that starts off the 16-byte grid
    assert_same_bits(one.cpu().numpy()[1:], want[1])
    assert one.cpu().numpy()[0] == sentinel


def test_run_argument_errors(amd):
    U, T, period, steps, Lc = 8, 65, 5, (-2, 1, 2), 40
    syn = amd.stream.Synthesizer(U, taps_of(T, 1), period, steps)
    W = syn.outputs(Lc)
    x = torch.from_numpy(noise((2, 3, Lc), 2)).cuda()
    with pytest.raises(TypeError):
        syn.run(x.cpu())                                       # no CPU fallback
    with pytest.raises(TypeError):
        syn.run(x.real.contiguous())
    with pytest.raises(ValueError):
        syn.run(x[:, :2])                                      # two channels for a bank of three
    with pytest.raises(ValueError):
        syn.run(x[0, 0])
    with pytest.raises(ValueError):
        syn.run(x[..., ::2])                                   # no unit sample stride
    with pytest.raises(ValueError):
        syn.run(x.transpose(0, 1).contiguous().transpose(0, 1))  # rows not C streams apart
    with pytest.raises(ValueError):
        syn.run(x, inv_scale=128.0)                            # inv_scale without dtype
    with pytest.raises(TypeError):
        syn.run(x, dtype=torch.int32)
    with pytest.raises(TypeError):
        syn.run(x, dtype=torch.float32)
    with pytest.raises(ValueError):
        syn.run(x, out=torch.empty((2, W - 1), dtype=torch.complex64, device="cuda"))
    with pytest.raises(ValueError):
        syn.run(x, out=torch.empty((3, W), dtype=torch.complex64, device="cuda"))
    with pytest.raises(ValueError):
        syn.run(x, out=torch.empty((2, W, 2), dtype=torch.complex64, device="cuda"))
    with pytest.raises(TypeError):
        syn.run(x, out=torch.empty((2, W), dtype=torch.float32, device="cuda"))
    with pytest.raises(TypeError):
        syn.run(x, out=torch.empty((2, W, 2), dtype=torch.int8, device="cuda"), dtype=torch.int16)
    with pytest.raises(ValueError):
        syn.run(x, out=torch.empty((2, W), dtype=torch.int8, device="cuda"), dtype=torch.int8)
    with pytest.raises(ValueError):
        syn.run(x, out=torch.empty((2, 2 * W), dtype=torch.complex64, device="cuda")[:, ::2])
    with pytest.raises(ValueError):
        syn.run(x, first_sample=-1)


def special_streams():
    """Two channels of 200 samples for (interp 3, ntaps 7, period 5, steps 1 and 2): NaN, +-inf and
    -0.0 among noise.  Where a NaN comes out, its sign and payload are the processor's."""
    x = noise((2, 200), 11)
    x[0, 3] = complex(np.inf, 0.25)
    x[0, 41] = complex(-0.5, -np.inf)
    x[0, 77] = complex(np.nan, 1.0)
    x[0, 140:170] = complex(-0.0, -0.0)
    x[1, 140:170] = complex(-0.0, -0.0)
    x[1, 100] = complex(np.inf, np.inf)
    x[1, 120] = complex(2.0, np.nan)
    x[1, 185] = complex(-np.inf, 3.0)
    return x


def test_nan_inf_and_negative_zero(amd):
    """An input with an inf and one with a NaN: they come out where the checker has them - every
    bit of every output that is not NaN, and NaN exactly where the checker's is - and the raw
    stores, which give NaN a code, equal the store rule everywhere."""
    U, T, period, steps = 3, 7, 5, (1, 2)
    h = taps_of(T, 12)
    x = special_streams()
    syn = amd.stream.Synthesizer(U, h, period, steps, (1.0, -1.0))
    xd = torch.from_numpy(x).cuda()
    got = syn.run(xd).cpu().numpy()
    want = sy.synthesize_host(x, h, U, steps, period, (1.0, -1.0))
    assert np.isnan(want.real).any() and np.isinf(want.real).any() and np.isinf(want.imag).any()
    assert_same_bits(got, want, nan_free=False)
    for dtype in RAW_DTYPES:
        codes = sy.store_host(want, NP_OF[dtype])
        assert np.array_equal(syn.run(xd, dtype=dtype).cpu().numpy(), codes)
        zero = sy.RAW[np.dtype(NP_OF[dtype])][4]
        assert (codes[np.isnan(want.real), 0] == zero).all()


@raw_param
def test_saturation_ties_and_nan_in_the_raw_store(amd, dtype):
    """One tap of 1.0, interp 1, one channel, gain 1 and an oscillator table of (1, 0): the outputs
    are the inputs (y = x*1 - x'*0), so the store rule meets chosen values: ties (k + 0.5 codes),
    values beyond both ends of the code range, infinities and NaN."""
    default, bias, lo, hi, zero = sy.RAW[np.dtype(NP_OF[dtype])]
    k = np.arange(-40, 40, dtype=np.float64)
    ties = (k + 0.5 - bias) / default                        # exact in fp32 for the power-of-two scales
    vals = np.concatenate([ties, [0.0, -0.0, 1.0, -1.0, 1.5, -1.5, 1e30, -1e30, (hi + 0.5 - bias) / default,
                                  (lo - 0.5 - bias) / default, (hi - 0.5 - bias) / default]])
    x = (vals + 1j * vals[::-1]).astype(np.complex64)[None, :]
    syn = amd.stream.Synthesizer(1, [1.0], 1, [0])
    y = syn.run(torch.from_numpy(x).cuda()).cpu().numpy()
    assert_same_bits(y, sy.synthesize_host(x, [1.0], 1, [0], 1))
    assert np.array_equal(y, x[0])  # (in value: a -0.0 comes out of the sums from +0.0 as +0.0)
    codes = sy.store_host(y, NP_OF[dtype])
    got = syn.run(torch.from_numpy(x).cuda(), dtype=dtype).cpu().numpy()
    assert np.array_equal(got, codes)
    assert (codes == lo).any() and (codes == hi).any()
    if bias == 0:   # the ties are exact: round half to even
        want = np.clip(np.where(np.floor(k) % 2 == 0, k, k + 1), lo, hi)
        assert np.array_equal(codes[:len(k), 0].astype(np.int64), want.astype(np.int64))
    # NaN and infinities: the imaginary part of the table is 0, so an infinite input makes a NaN
    # in the other component (inf * 0); the codes are the store rule's on the host model
    s = np.array([[complex(np.nan, 0.5), complex(np.inf, 0.25), complex(0.25, -np.inf), complex(0.5, 0.5)]],
                 np.complex64)
    want = sy.synthesize_host(s, [1.0], 1, [0], 1)
    assert np.isnan(want.real).any() and np.isinf(want.real).any()
    got = syn.run(torch.from_numpy(s).cuda(), dtype=dtype).cpu().numpy()
    assert np.array_equal(got, sy.store_host(want, NP_OF[dtype]))
    assert got[0, 0] == zero and got[1, 0] == hi


def test_raw_store_agrees_with_quantize_at_power_of_two_scales(amd):
    """What the header claims about iq_io.quantize: equal codes for the cs16 and cs8 defaults."""
    i = 14
    U, T, period, steps, gains, _ = SHAPES[i]
    x, h, want = shape_case(i)
    syn = amd.stream.Synthesizer(U, h, period, steps, gains)
    xd = torch.from_numpy(x).cuda()
    y = syn.run(xd)
    for dtype in (torch.int16, torch.int8):
        assert torch.equal(syn.run(xd, dtype=dtype), amd.iq_io.quantize(y, dtype))


@pytest.mark.parametrize("dtype", [None, torch.int16], ids=["complex64", "cs16"])
def test_one_run_captured_in_a_graph_replays_the_eager_bits(amd, dtype):
    U, T, period, steps, Lc = 8, 65, 5, (-2, 1, 2), 9 + 200
    h = taps_of(T, 31)
    syn = amd.stream.Synthesizer(U, h, period, steps, (1.0, 0.5, 0.1))
    dev = torch.from_numpy(noise((3, Lc), 32)).cuda()
    dev2 = torch.from_numpy(noise((3, Lc), 33)).cuda()
    eager = syn.run(dev, first_sample=7, dtype=dtype).cpu().numpy()
    eager2 = syn.run(dev2, first_sample=7, dtype=dtype).cpu().numpy()
    out = torch.zeros(eager.shape, dtype=dtype or torch.complex64, device="cuda")
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        syn.run(dev, first_sample=7, out=out, dtype=dtype)  # warm the stream-side state before capture
    torch.cuda.current_stream().wait_stream(s)
    out.zero_()
    with torch.cuda.graph(g):
        syn.run(dev, first_sample=7, out=out, dtype=dtype)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint8), eager.view(np.uint8))
    dev.copy_(dev2)  # new samples in the captured buffer
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint8), eager2.view(np.uint8))


# ---- the wideband transmit chain, looped back ------------------------------------------------

@functools.lru_cache(maxsize=None)
def loopback_case():
    """CONFIGS[0]'s planted frames: (symbols [K, S], channel [K], starts [K], chan_len)."""
    from oracle.pyoracle import Oracle

    chans, planted = sy.planted_channels(Oracle(), 0)
    channel = np.concatenate([np.full(len(s), c, np.int64) for c, (s, _) in enumerate(planted)])
    starts = np.concatenate([s for s, _ in planted])
    syms = np.concatenate([y for _, y in planted])
    return syms, channel, starts, chans.shape[1]


@pytest.mark.parametrize("dtype", [None] + RAW_DTYPES, ids=["complex64", "cs16", "cs8", "cu8"])
def test_work_wideband_into_receive_wideband_returns_what_was_planted(amd, dtype):
    """LoRaMod.work_wideband -> receive_wideband on CONFIGS[0]: the frames come back in their
    channels, their starts moved by the two banks' delays, with their symbols.  The gains keep the
    sum of the five channels inside the raw formats' range (5 * 0.15 with room for the filter's
    overshoot at the frames' edges); the complex64 case uses the configuration's near-far amps."""
    sf, osr, D, period, T, cutoff, rows, steps, amps = cc.CONFIGS[0]
    syms, channel, starts, chan_len = loopback_case()
    gains = amps[1] if dtype is None else (0.15,) * len(steps)
    syn = amd.stream.Synthesizer(D, amd.stream.lowpass_taps(T, 0.5 / D, gain=D), period, steps, gains)
    mod = amd.LoRaMod(sf, ovs=osr)
    x = mod.work_wideband(syn, torch.from_numpy(syms.astype(np.int32)), channel, starts, chan_len, dtype=dtype)
    assert x.shape == ((syn.outputs(chan_len),) if dtype is None else (syn.outputs(chan_len), 2))
    assert x.dtype == (dtype or torch.complex64)
    if dtype is not None:   # nothing clipped
        lo, hi = sy.RAW[np.dtype(NP_OF[dtype])][2:4]
        assert int(x.min()) > lo and int(x.max()) < hi
    plan = amd.DemodPlan(sf, osr, dechirp=True)
    chan = amd.stream.Channelizer(D, amd.stream.lowpass_taps(T, cutoff), period, steps)
    got_ch, got_st, res = amd.stream.receive_wideband(plan, chan, x, syms.shape[1])
    torch.cuda.synchronize()
    shift = sy.loopback_shift(T, D, T, D)
    assert shift == -8
    assert got_ch.cpu().tolist() == channel.tolist()
    assert got_st.cpu().tolist() == (starts + shift).tolist()
    assert np.array_equal(res.symbols.cpu().numpy() % (1 << sf), syms)
    assert (res.sync.cpu().numpy() == 0x12).all()


def test_work_wideband_into_the_demod_blocks_work_wideband(amd):
    sf, osr, D, period, T, cutoff, rows, steps, amps = cc.CONFIGS[0]
    syms, channel, starts, chan_len = loopback_case()
    syn = amd.stream.Synthesizer(D, amd.stream.lowpass_taps(T, 0.5 / D, gain=D), period, steps)
    x = amd.LoRaMod(sf, ovs=osr).work_wideband(syn, torch.from_numpy(syms.astype(np.int32)), channel, starts,
                                               chan_len)
    demod = amd.LoRaDemod(sf, osr=osr)
    chan = amd.stream.Channelizer(D, amd.stream.lowpass_taps(T, cutoff), period, steps)
    got_ch, got_st, got = demod.work_wideband(chan, x, syms.shape[1])
    torch.cuda.synchronize()
    assert got_ch.cpu().tolist() == channel.tolist() and got_st.cpu().tolist() == (starts - 8).tolist()
    assert np.array_equal(got.cpu().numpy()[:, :syms.shape[1]] % (1 << sf), syms)
    assert demod.sync_ok().all()


def test_transmit_wideband_places_frames_and_refuses_overlaps(amd):
    U, T, period, steps = 4, 17, 5, (1, -1)
    h = sy.lowpass_taps(T, 0.5 / U, U)
    syn = amd.stream.Synthesizer(U, h, period, steps, (1.0, 0.5))
    frames = noise((3, 20), 8)
    fd = torch.from_numpy(frames).cuda()
    chans = np.zeros((2, 100), np.complex64)
    chans[0, 5:25], chans[1, 0:20], chans[0, 25:45] = frames[0], frames[1], frames[2]
    got = amd.stream.transmit_wideband(syn, fd, [0, 1, 0], [5, 0, 25], 100, first_sample=9)
    assert_same_bits(got.cpu().numpy(), sy.synthesize_host(chans, h, U, steps, period, (1.0, 0.5), first_sample=9))
    raw = amd.stream.transmit_wideband(syn, fd, torch.tensor([0, 1, 0]), torch.tensor([5, 0, 25]), 100,
                                       dtype=torch.int8, inv_scale=16.0)
    want = sy.store_host(sy.synthesize_host(chans, h, U, steps, period, (1.0, 0.5)), np.int8, 16.0)
    assert np.array_equal(raw.cpu().numpy(), want)
    for ch, st in (([0, 1, 0], [5, 0, 24]), ([0, 0, 0], [5, 5, 40]), ([0, 2, 0], [5, 0, 25]), ([0, 1, 0], [5, 0, 81]),
                   ([0, 1, 0], [-1, 0, 25]), ([0, 1], [5, 0])):
        with pytest.raises(ValueError):
            amd.stream.transmit_wideband(syn, fd, ch, st, 100)
    empty = amd.stream.transmit_wideband(syn, fd[:0], [], [], 100)
    assert empty.shape == (syn.outputs(100),) and not empty.cpu().numpy().any()
