"""GPU: the channel impairment stage (lora_phy_amd.stream.impair, lora_impair_batch and
lora_impair_raw_batch) against the numpy restatement of its definition (tests/impair_checker.py):
every comparison is ``==`` on the bits.  The shapes are the smallest at which the kernel can go
wrong: a workgroup owns 1024 samples of a row and a lane a pair of them, so the lengths sit round
one tile and two, the views start on even and odd samples, and first_sample is even and odd."""
import functools

import numpy as np
import pytest

from tests import channel_checker as cc
from tests import impair_checker as ic
from tests import scan_checker as sc
from tests import synth_checker as sy

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NP_OF = {torch.int16: np.int16, torch.int8: np.int8, torch.uint8: np.uint8}
RAW_DTYPES = [torch.int16, torch.int8, torch.uint8]
SENTINEL = 12345.0


@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import lora_phy_amd

    return lora_phy_amd


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def samples(rows, L, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((rows, L)) + 1j * rng.standard_normal((rows, L))).astype(np.complex64)


def dev_params(kw):
    """The checker's keyword arguments as ``impair``'s: per-row lists become device tensors (int32
    words for fcw and phase), fcw is called cfo there."""
    out = {}
    for k, v in kw.items():
        name = "cfo" if k == "fcw" else k
        if k in ("gain", "sigma") and v is not None:
            v = torch.tensor(np.asarray(v, np.float32).reshape(-1)).cuda()
        elif k in ("fcw", "phase") and v is not None:
            v = torch.tensor(np.asarray(v, np.int64).astype(np.int32).reshape(-1)).cuda()
        out[name] = v
    return out


def run(amd, x, in_off=0, out_off=0, pad=3, dtype=None, inplace=False, rows=None, length=None, **kw):
    """``impair`` on views of larger buffers: row r of the input begins ``in_off + r * (L + pad)``
    samples into its buffer, of the output ``out_off + r * (L + pad + 2)`` samples into its own,
    which is filled with a sentinel first; everything outside the rows must still hold it.
    Returns the result as numpy (complex64 [R, L], or codes [R, L, 2])."""
    if x is None:
        R, L = rows, length
        xin = None
    else:
        R, L = x.shape
        si = L + pad
        buf = torch.zeros(in_off + R * si + 1, dtype=torch.complex64, device="cuda")
        xin = buf[in_off:in_off + R * si].view(R, si)[:, :L]
        xin.copy_(torch.from_numpy(x).cuda())
    if inplace:
        got = amd.stream.impair(xin, out=xin, **dev_params(kw))
        assert got.data_ptr() == xin.data_ptr()
        torch.cuda.synchronize()
        return got.cpu().numpy()
    so = L + pad + 2
    tail = () if dtype is None else (2,)

    def rows_of(buf):
        return buf[out_off:out_off + R * so].view(R, so, *tail)[:, :L]

    if dtype is None:
        obuf = torch.full((out_off + R * so + 1,), SENTINEL, dtype=torch.complex64, device="cuda")
    else:
        obuf = torch.full((out_off + R * so + 1, 2), 77, dtype=dtype, device="cuda")
    before = obuf.clone()
    out = rows_of(obuf)
    extra = {} if x is not None else dict(rows=R, length=L)
    got = amd.stream.impair(xin, out=out, dtype=dtype, **extra, **dev_params(kw))
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and got.shape == out.shape
    res = got.cpu().numpy().copy()
    out.copy_(rows_of(before))
    assert torch.equal(obuf.view(torch.uint8), before.view(torch.uint8)), "a sample outside the rows was written"
    return res


ALL = dict(gain=[1.5, 0.5, -2.0], fcw=[ic.cfo_word(0.25 / 128), -123456789, 1 << 30], phase=[7, -(1 << 31), 99],
           sigma=[0.25, 1.0, 0.0625], seed=(9 << 32) | 2026)


def first_rows(kw, R):
    return {k: (v[:R] if isinstance(v, list) else v) for k, v in kw.items()}


@pytest.mark.parametrize("L", [1, 2, 3, 1023, 1024, 1025, 2049])
def test_lengths_rows_and_views(amd, L):
    """Rows 1 and 3 with strides greater than row_len, views that start on an odd sample for in,
    for out and for both, first_sample even and odd (the shared-block path and the two-block
    path at both alignments)."""
    x = samples(3, L, 100 + L)
    for first in (6, 7):
        want = ic.impair_host(x, first_sample=first, first_row=3, **ALL)
        for in_off, out_off in ((0, 0), (1, 0), (0, 1), (1, 1)):
            got = run(amd, x, in_off, out_off, first_sample=first, first_row=3, **ALL)
            assert (bits(got) == bits(want)).all(), (L, first, in_off, out_off)
        one = run(amd, x[:1], 1, 0, first_sample=first, first_row=3, **first_rows(ALL, 1))
        assert (bits(one) == bits(want[:1])).all(), (L, first)
    # an odd stride puts the rows at both alignments in one launch
    got = run(amd, x, 0, 0, pad=4, first_sample=7, first_row=3, **ALL)
    assert (bits(got) == bits(want)).all()


def test_64_bit_boundaries(amd):
    x = samples(3, 8, 5)
    kw = dict(fcw=[ic.cfo_word(0.01)] * 3, phase=[5] * 3, sigma=[0.25] * 3, seed=11)
    for first in ((1 << 32) - 3, (1 << 33) - 3):  # the phase word wraps, the block counter's high word begins
        for off in (0, 1):
            got = run(amd, x, off, off, first_sample=first, **kw)
            assert (bits(got) == bits(ic.impair_host(x, first_sample=first, **kw))).all(), (first, off)
    got = run(amd, x, first_row=(1 << 32) - 2, **kw)
    assert (bits(got) == bits(ic.impair_host(x, first_row=(1 << 32) - 2, **kw))).all()
    # seeds that differ only above bit 31
    a = run(amd, None, rows=1, length=8, sigma=[1.0], seed=3)
    b = run(amd, None, rows=1, length=8, sigma=[1.0], seed=3 | (1 << 32))
    assert not (a == b).any()
    assert (bits(a) == bits(ic.impair_host(None, 1, 8, sigma=1.0, seed=3))).all()
    assert (bits(b) == bits(ic.impair_host(None, 1, 8, sigma=1.0, seed=3 | (1 << 32)))).all()


STAGES = {
    "gain": dict(gain=[1.5, 0.5, -2.0, 0.0]),
    "fcw": dict(fcw=[0, 1, -1, -(1 << 31)]),
    "phase": dict(phase=[0, 1, -1, -(1 << 31)]),
    "fcw+phase": dict(fcw=[0, 1, -1, -(1 << 31)], phase=[3, 1 << 30, -(1 << 31), 12345]),
    "sigma": dict(sigma=[0.0, 0.5, 1.0, 4.0], seed=5),
    "gain+fcw": dict(gain=[1.5, 0.5, -2.0, 0.0], fcw=[0, 1, -1, -(1 << 31)]),
    "gain+sigma": dict(gain=[1.5, 0.5, -2.0, 0.0], sigma=[0.0, 0.5, 1.0, 4.0], seed=5),
    "fcw+sigma": dict(fcw=[12345678, 1, -1, -(1 << 31)], sigma=[0.0, 0.5, 1.0, 4.0], seed=5),
    "all": dict(gain=[1.5, 0.5, -2.0, 0.0], fcw=[0, 1, -1, -(1 << 31)], phase=[3, 1 << 30, -(1 << 31), 12345],
                sigma=[0.0, 0.5, 1.0, 4.0], seed=5),
}


@pytest.mark.parametrize("name", sorted(STAGES))
def test_each_stage_alone_and_all_together(amd, name):
    """A NULL array of each kind: the stage is not performed.  Row 0 holds -0.0 components, which
    a neutral rotation or an added zero would turn into +0.0."""
    x = samples(4, 37, 8)
    x[:, :4] = np.array([-0.0, -0.0, 1.0, -0.0, -0.0, 2.0, 0.0, 0.0], np.float32).view(np.complex64)
    kw = STAGES[name]
    for first in (1000, 1001):
        got = run(amd, x, 1, 0, first_sample=first, **kw)
        assert (bits(got) == bits(ic.impair_host(x, first_sample=first, **kw))).all(), (name, first)


def test_noise_only_rows(amd):
    for first in (0, 1):
        got = run(amd, None, out_off=first, rows=3, length=1025, sigma=[0.5, 0.0, 2.0], seed=77, first_sample=first,
                  first_row=9)
        want = ic.impair_host(None, 3, 1025, sigma=[0.5, 0.0, 2.0], seed=77, first_sample=first, first_row=9)
        assert (bits(got) == bits(want)).all()
    one = amd.stream.impair(None, sigma=0.5, seed=77, length=16, first_row=9)
    assert one.shape == (16,)
    assert (bits(one.cpu().numpy()) == bits(ic.impair_host(None, 1, 16, sigma=0.5, seed=77, first_row=9)[0])).all()


@functools.lru_cache(maxsize=None)
def split_case():
    x = samples(3, 2049, 21)
    return x, ic.impair_host(x, first_sample=12345, first_row=40, **ALL)


def test_one_call_equals_its_splits(amd):
    x, want = split_case()
    whole = run(amd, x, first_sample=12345, first_row=40, **ALL)
    assert (bits(whole) == bits(want)).all()
    cut = 1001
    a = run(amd, np.ascontiguousarray(x[:, :cut]), first_sample=12345, first_row=40, **ALL)
    b = run(amd, np.ascontiguousarray(x[:, cut:]), first_sample=12345 + cut, first_row=40, **ALL)
    assert (bits(np.concatenate([a, b], axis=1)) == bits(whole)).all()
    for r in range(3):
        kw = {k: (v[r:r + 1] if isinstance(v, list) else v) for k, v in ALL.items()}
        one = run(amd, x[r:r + 1], first_sample=12345, first_row=40 + r, **kw)
        assert (bits(one) == bits(whole[r:r + 1])).all(), r


def test_in_place_equals_out_of_place(amd):
    x, want = split_case()
    for off in (0, 1):
        got = run(amd, x, in_off=off, inplace=True, first_sample=12345, first_row=40, **ALL)
        assert (bits(got) == bits(want)).all(), off


@pytest.mark.parametrize("dtype", RAW_DTYPES, ids=["cs16", "cs8", "cu8"])
def test_raw_formats_equal_the_store_rule(amd, dtype):
    """sigma 0.5 on samples of deviation 0.5 a component: some codes clip at the default scale."""
    x = (0.5 * samples(3, 1027, 33)).astype(np.complex64)
    kw = dict(gain=[1.0, 0.5, 2.0], fcw=[5, -77777, 1 << 29], sigma=[0.5, 0.25, 1.0], seed=4, first_sample=3)
    flt = run(amd, x, **kw)
    want = sy.store_host(flt, NP_OF[dtype])
    assert (want == ic.impair_raw_host(x, NP_OF[dtype], **kw)).all()
    lo, hi = sy.RAW[np.dtype(NP_OF[dtype])][2:4]
    assert (want == lo).any() and (want == hi).any()  # clipped both ways
    for in_off, out_off in ((0, 0), (0, 1), (1, 1), (1, 2), (0, 3)):
        got = run(amd, x, in_off, out_off, dtype=dtype, **kw)
        assert got.dtype == NP_OF[dtype] and (got == want).all(), (in_off, out_off)
    # another scale, and noise-only rows
    got = run(amd, None, out_off=1, dtype=dtype, rows=2, length=1025, sigma=[0.3, 1.0], seed=8, scale=100.0)
    want = sy.store_host(ic.impair_host(None, 2, 1025, sigma=[0.3, 1.0], seed=8), NP_OF[dtype], 100.0)
    assert (got == want).all()


def test_nan_and_inf_propagate_as_the_checker_says(amd):
    x = samples(2, 40, 44)
    x[0, 3] = complex(np.nan, 1.0)
    x[0, 4] = complex(np.inf, 1.0)
    x[0, 5] = complex(1.0, -np.inf)
    x[1, 6] = complex(np.inf, np.inf)
    x[1, 7] = complex(np.nan, np.nan)
    kw = dict(gain=[2.0, 0.0], fcw=[1 << 28, 1 << 30], sigma=[0.5, 0.5], seed=1)
    for dtype in [None] + RAW_DTYPES:
        got = run(amd, x, 1, 1, dtype=dtype, **kw)
        want = ic.impair_host(x, **kw)
        if dtype is not None:
            assert (got == sy.store_host(want, NP_OF[dtype])).all()  # a NaN stores the format's zero
            continue
        g, w = got.view(np.float32), want.view(np.float32)
        assert np.isnan(w).sum() >= 6 and np.isinf(w).any()
        assert (np.isnan(g) == np.isnan(w)).all()
        assert (bits(np.nan_to_num(g, nan=0.0, posinf=np.inf, neginf=-np.inf)) ==
                bits(np.nan_to_num(w, nan=0.0, posinf=np.inf, neginf=-np.inf))).all()


def test_scalars_snr_and_cycles(amd):
    """The Python conveniences: scalars for every row, snr_db through noise_sigma, cfo and phase in
    cycles through cfo_word, float tensors converted on the device."""
    x = samples(2, 100, 55)
    xd = torch.from_numpy(x).cuda()
    got = amd.stream.impair(xd, snr_db=5.0, amplitude=2.0, cfo=0.25 / 128, phase=0.125, gain=0.5, seed=6)
    want = ic.impair_host(x, sigma=amd.stream.noise_sigma(5.0, 2.0), fcw=ic.cfo_word(0.25 / 128),
                          phase=ic.cfo_word(0.125), gain=0.5, seed=6)
    assert (bits(got.cpu().numpy()) == bits(want)).all()
    cyc = torch.tensor([0.25 / 128, -0.3], dtype=torch.float64, device="cuda")
    got = amd.stream.impair(xd, cfo=cyc)
    want = ic.impair_host(x, fcw=[ic.cfo_word(0.25 / 128), ic.cfo_word(-0.3)])
    assert (bits(got.cpu().numpy()) == bits(want)).all()
    assert (bits(amd.stream.impair(xd[0], gain=3.0).cpu().numpy()) == bits(ic.impair_host(x[0], gain=3.0))).all()
    with pytest.raises(ValueError):
        amd.stream.impair(xd)
    with pytest.raises(ValueError):
        amd.stream.impair(xd, gain=torch.ones(3, device="cuda"))
    assert amd.stream.impair(xd[:, :0], gain=1.0).shape == (2, 0)


def test_loopback_through_stream_receive(amd):
    """Three SF7 frames at osr 1 planted with gaps, impaired at +5 dB with a carrier offset of a
    quarter bin: ``receive`` returns the planted starts, and its symbols equal the oracle's on the
    same noisy samples copied back."""
    from oracle.pyoracle import Oracle

    O = Oracle()
    sf, S, gaps = 7, 16, (37, 301, 500)
    N = 1 << sf
    frame_len = (S + 2) * N
    starts, L = sc.planted_layout(sf, 1, S, gaps)
    L += 300
    rng = np.random.default_rng(71)
    syms = rng.integers(0, N, (len(gaps), S)).astype(np.uint16)
    frames = amd.modulate(torch.from_numpy(syms.astype(np.int32)).cuda(), sf, 1, 125000, 1.0, 0x12)
    x = torch.zeros(L, dtype=torch.complex64, device="cuda")
    for s, f in zip(starts.tolist(), frames):
        x[s:s + frame_len] = f
    y = amd.stream.impair(x, snr_db=5.0, cfo=0.25 / N, seed=2026)
    plan = amd.DemodPlan(sf, dechirp=True)
    got_starts, res = amd.stream.receive(plan, y, S)
    torch.cuda.synchronize()
    assert got_starts.cpu().tolist() == starts.tolist()
    host = y.cpu().numpy()
    assert (bits(host) == bits(ic.impair_host(x.cpu().numpy(), sigma=amd.stream.noise_sigma(5.0),
                                              fcw=ic.cfo_word(0.25 / N), seed=2026))).all()
    cut = np.stack([host[s:s + frame_len] for s in starts])
    o_syms, o_sync, o_cfo, o_toff, cnt = O.demod_frames(cut, sf, 1, False, True)
    assert (np.asarray(cnt) == S).all()
    assert np.array_equal(res.symbols.cpu().numpy(), np.asarray(o_syms)[:, :S])
    assert np.array_equal(res.sync.cpu().numpy(), np.asarray(o_sync).astype(np.uint8))


def test_wideband_loopback_through_cu8(amd):
    """transmit_wideband -> impair(dtype=uint8) -> receive_wideband on channel_checker's smallest
    configuration: the planted starts come back (moved by the two banks' delays)."""
    from oracle.pyoracle import Oracle

    sf, osr, D, period, T, cutoff, rows, steps, amps = cc.CONFIGS[0]
    chans, planted = sy.planted_channels(Oracle(), 0)
    channel = np.concatenate([np.full(len(s), c, np.int64) for c, (s, _) in enumerate(planted)])
    starts = np.concatenate([s for s, _ in planted])
    syms = np.concatenate([y for _, y in planted])
    syn = amd.stream.Synthesizer(D, amd.stream.lowpass_taps(T, 0.5 / D, gain=D), period, steps,
                                 (0.15,) * len(steps))
    frames = amd.modulate(torch.from_numpy(syms.astype(np.int32)).cuda(), sf, osr, 125000, 1.0, 0x12)
    wide = amd.stream.transmit_wideband(syn, frames, channel, starts, chans.shape[1])
    raw = amd.stream.impair(wide, sigma=0.02, seed=5, dtype=torch.uint8)
    assert raw.shape == (wide.shape[0], 2) and raw.dtype == torch.uint8
    plan = amd.DemodPlan(sf, osr, dechirp=True)
    chan = amd.stream.Channelizer(D, amd.stream.lowpass_taps(T, cutoff), period, steps)
    got_ch, got_st, res = amd.stream.receive_wideband(plan, chan, raw, syms.shape[1])
    torch.cuda.synchronize()
    assert got_ch.cpu().tolist() == channel.tolist()
    assert got_st.cpu().tolist() == (starts + sy.loopback_shift(T, D, T, D)).tolist()
    assert np.array_equal(res.symbols.cpu().numpy() % (1 << sf), syms)


def test_device_guard(amd):
    """On a second device the call leaves the current device unchanged and computes there what it
    computes on device 0."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two HIP devices")
    torch.cuda.set_device(0)
    x = torch.from_numpy(samples(2, 65, 3))
    outs = []
    for d in (1, 0):
        y = amd.stream.impair(x.to(f"cuda:{d}"), sigma=0.5, cfo=0.01, gain=2.0, seed=9)
        n = amd.stream.impair(None, sigma=0.5, seed=9, length=33, device=f"cuda:{d}")
        assert torch.cuda.current_device() == 0
        torch.cuda.synchronize(d)
        assert y.device.index == d and n.device.index == d
        outs.append((y.cpu(), n.cpu()))
    for g, w in zip(*outs):
        assert g.numel() > 0 and torch.equal(torch.view_as_real(g).view(torch.int32),
                                             torch.view_as_real(w).view(torch.int32))


def test_sweep_receive_counts_what_was_planted(amd):
    """awgn.sweep_receive at a high SNR finds every planted frame with every symbol right, with and
    without a quarter-bin carrier offset; its noise is impair's, so a second run gives the same
    counts; and the noise-only record counts windows."""
    from lora_phy_amd import awgn

    for cfo in (0.0, 0.25):
        recs = awgn.sweep_receive(7, [15.0, -30.0], frames=10, frame_symbols=6, cfo_bins=cfo, seed=3,
                                  noise_windows=2000, noise_batch_samples=1 << 16)
        assert [r.get("snr_db") for r in recs] == [15.0, -30.0, None] and recs[2]["noise_only"]
        hi, lo, noise = recs
        assert hi["planted"] == 12 and hi["detected"] == 12 and hi["all_symbols_correct"] == 12
        assert hi["false_starts"] == 0 and hi["p_detect"] == 1.0 and hi["p_all_correct_given_detected"] == 1.0
        assert lo["planted"] == 12 and 0 <= lo["detected"] <= 12 and lo["all_symbols_correct"] <= lo["detected"]
        assert noise["windows"] >= 2000 and noise["false_starts"] >= 0
        again = awgn.sweep_receive(7, [15.0, -30.0], frames=10, frame_symbols=6, cfo_bins=cfo, seed=3)
        assert again == recs[:2]
