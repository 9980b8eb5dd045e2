"""GPU: the frame finder on the device (lora_find_frames_batch through
lora_phy_amd.stream.find_frames_device) and the stream receive built on it (receive_device,
receive_wideband_device, LoRaDemod.work_stream_device / work_wideband_device).

Expected values never come from the new code: count, starts and end are those of the numpy
restatement of the rule (tests/scan_checker.find_frames_host), integer for integer, and the
receive chains are compared with the unchanged host-finder chains (stream.receive,
receive_wideband) bit for bit.

The finder reads three arrays only, so most of this file feeds it synthetic metrics that stress
the greedy pass far harder than planted frames do: hundreds of accepted frames and thousands of
candidates per row, most of them rejected because they start before `first`, with NaN power and
-inf floors sprinkled in.  A wrong pass cannot agree by accident."""
import functools

import numpy as np
import pytest

from tests import channel_checker as cc
from tests import detect_checker as dc
from tests import resample_checker as rc
from tests import scan_checker as sc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SYNC = 0x12


@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import lora_phy_amd

    return lora_phy_amd


# ---- synthetic metrics -----------------------------------------------------------------------

def tile():
    from lora_phy_amd import _capi

    return _capi.FIND_TILE


def cases():
    """(sf, osr, k, W, frac, frame_symbols); the last one carries the pass's state across two of
    the kernel's own tile boundaries and ends in a partial tile."""
    return [(7, 1, 4, 8229, 0.2, 1), (7, 1, 4, 8229, 0.2, 6), (6, 2, 8, 8229, 0.5, 0), (12, 1, 2, 8229, 0.3, 1),
            (9, 1, 512, 20000, 0.3, 2), (7, 1, 4, 2 * tile() + 37, 0.3, 1)]


NCASES = 6


@functools.lru_cache(maxsize=None)
def synthetic(seed, sf, k, W, frac, sync=SYNC):
    rng = np.random.default_rng(seed)
    N = 1 << sf
    sw0, sw1 = (sync >> 4) << (sf - 4), (sync & 15) << (sf - 4)
    index = rng.integers(0, N, W)
    if W > k:
        for w in np.flatnonzero(rng.random(W - k) < frac):  # in increasing w: chains build up
            index[w + k] = (index[w] + sw1 - sw0) % N
    power = rng.normal(0, 3, W).astype(np.float32)
    power_avg = (power - rng.normal(2, 3, W).astype(np.float32)).astype(np.float32)
    power[rng.random(W) < 0.01] = np.nan
    power_avg[rng.random(W) < 0.01] = -np.inf
    m = {"index": index.astype(np.uint16), "power": power, "power_avg": power_avg}
    for v in m.values():
        v.setflags(write=False)
    return m


def variants(W, hop, step):
    """(first, row_len, thresh_db): the defaults, and a pass that starts late, ends early and
    gates harder."""
    return [(0, None, 0.0), (1000, (W - 1) * hop - 3 * hop, 1.5)]


def expected(m, hop, sf, osr, fs, thresh_db, first, row_len, capacity=None, sync=SYNC):
    """(count, starts padded or cut to capacity, end) by the host model."""
    step = (1 << sf) * osr
    frame_len = (fs + 2) * step
    W = len(m["index"])
    if row_len is None:
        row_len = (W - 1) * hop + step if W else 0
    got = sc.find_frames_host(m, hop, sf, osr, fs, sync, thresh_db, first, row_len)
    if capacity is None:
        capacity = row_len // frame_len
    starts = np.full(capacity, -1, np.int64)
    starts[:min(len(got), capacity)] = got[:capacity]
    return len(got), starts, int(got[-1]) + frame_len if len(got) else first


def to_device(amd, ms, stride=None):
    """DetectMetrics of the rows `ms` (equal W) on the device, rows `stride` columns apart."""
    W = len(ms[0]["index"])
    stride = W if stride is None else stride

    def put(key, fill):
        buf = np.full((len(ms), stride), fill, ms[0][key].dtype)
        for r, m in enumerate(ms):
            buf[r, :W] = m[key]
        return torch.from_numpy(buf).cuda()[:, :W]

    # what lies between the rows would pass every test if it were read: +inf power, peak sw0
    return amd.DetectMetrics(put("power", np.inf), put("power_avg", 0), None, put("index", 0))


def check(found, want):
    """found (FoundFrames, on the device) against [(count, starts, end)] per row."""
    torch.cuda.synchronize()
    assert found.count.dtype == torch.int32 and found.starts.dtype == found.end.dtype == torch.int64
    count, starts, end = found.count.cpu().numpy(), found.starts.cpu().numpy(), found.end.cpu().numpy()
    assert count.shape == end.shape == (len(want),) and starts.shape == (len(want), len(want[0][1]))
    for r, (c, s, e) in enumerate(want):
        assert count[r] == c, (r, count[r], c)
        assert np.array_equal(starts[r], s), (r, np.flatnonzero(starts[r] != s)[:5])
        assert end[r] == e, (r, end[r], e)
    valid = found.valid.cpu().numpy()
    assert np.array_equal(valid, np.arange(starts.shape[1])[None, :] < count[:, None])


@pytest.mark.parametrize("vi", [0, 1])
@pytest.mark.parametrize("ci", range(NCASES))
def test_single_row_equals_the_host_model(amd, ci, vi):
    sf, osr, k, W, frac, fs = cases()[ci]
    step = (1 << sf) * osr
    hop = step // k
    first, row_len, thresh = variants(W, hop, step)[vi]
    m = synthetic(100 + ci, sf, k, W, frac)
    want = expected(m, hop, sf, osr, fs, thresh, first, row_len)
    assert want[0] >= 9  # the pass has work to do (9 to several hundred frames)
    met = to_device(amd, [m])
    found = amd.stream.find_frames_device(met, hop, sf, osr, fs, SYNC, thresh, first, row_len)
    check(found, [want])
    # a [W] input is one row
    one = amd.DetectMetrics(met.power[0], met.power_avg[0], None, met.index[0])
    check(amd.stream.find_frames_device(one, hop, sf, osr, fs, SYNC, thresh, first, row_len), [want])


@pytest.mark.parametrize("ci", range(NCASES))
def test_batch_with_a_first_per_row_and_strided_rows(amd, ci):
    """Five rows of different seeds, a different `first` per row (a device tensor), rows further
    apart than W; the same batch with one int `first` for all rows."""
    sf, osr, k, W, frac, fs = cases()[ci]
    step = (1 << sf) * osr
    hop = step // k
    R = 5
    ms = [synthetic(200 + 10 * ci + r, sf, k, W, frac) for r in range(R)]
    firsts = [0, 1, step // 2 + 1, 1000, (W // 2) * hop + 3]
    _, row_len, thresh = variants(W, hop, step)[1]
    want = [expected(m, hop, sf, osr, fs, thresh, f, row_len) for m, f in zip(ms, firsts)]
    assert len({w[0] for w in want}) > 1  # the rows differ
    met = to_device(amd, ms, stride=W + 13)
    assert met.power.stride(0) == W + 13
    first_t = torch.tensor(firsts, dtype=torch.int64).cuda()
    check(amd.stream.find_frames_device(met, hop, sf, osr, fs, SYNC, thresh, first_t, row_len), want)
    want = [expected(m, hop, sf, osr, fs, thresh, 1000, row_len) for m in ms]
    check(amd.stream.find_frames_device(met, hop, sf, osr, fs, SYNC, thresh, 1000, row_len), want)


def test_all_nan_power_and_rows_with_no_window_to_test(amd):
    sf, osr, k, W, frac, fs = cases()[0]
    hop = (1 << sf) * osr // k
    m = dict(synthetic(100, sf, k, W, frac))
    m["power"] = np.full(W, np.nan, np.float32)
    want = expected(m, hop, sf, osr, fs, 0.0, 0, None)
    assert want[0] == 0 and want[2] == 0 and (want[1] == -1).all() and len(want[1]) > 0
    check(amd.stream.find_frames_device(to_device(amd, [synthetic(100, sf, k, W, frac), m]), hop, sf, osr, fs),
          [expected(synthetic(100, sf, k, W, frac), hop, sf, osr, fs, 0.0, 0, None), want])
    # W <= k: nothing to test, everything still written (first = 77 comes back as end)
    for W2 in (k, k - 1, 1, 0):
        ms = [{key: v[:W2] for key, v in synthetic(100, sf, k, W, frac).items()}] * 2
        met = to_device(amd, ms)
        found = amd.stream.find_frames_device(met, hop, sf, osr, fs, first=77, row_len=5000, capacity=4)
        check(found, [(0, np.full(4, -1, np.int64), 77)] * 2)
    # no row at all: empty outputs, no launch
    none = amd.DetectMetrics(*(torch.empty((0, 9), dtype=dt, device="cuda")
                               for dt in (torch.float32, torch.float32, torch.float32, torch.uint16)))
    found = amd.stream.find_frames_device(none, hop, sf, osr, fs)
    assert found.count.shape == found.end.shape == (0,) and found.starts.shape[0] == 0


@pytest.mark.parametrize("ci", [0, 4, 5])
def test_capacity_below_above_and_zero_and_out(amd, ci):
    sf, osr, k, W, frac, fs = cases()[ci]
    step = (1 << sf) * osr
    hop = step // k
    ms = [synthetic(100 + ci, sf, k, W, frac), synthetic(300 + ci, sf, k, W, frac)]
    met = to_device(amd, ms)
    full = [expected(m, hop, sf, osr, fs, 0.0, 0, None) for m in ms]
    lo = min(w[0] for w in full)
    assert lo >= 5
    for cap in (lo - 3, max(w[0] for w in full) + 7, 0, 1):
        want = [expected(m, hop, sf, osr, fs, 0.0, 0, None, capacity=cap) for m in ms]
        found = amd.stream.find_frames_device(met, hop, sf, osr, fs, capacity=cap)
        check(found, want)
        count, starts = found.count.cpu().numpy(), found.starts.cpu().numpy()
        assert [int(c) for c in count] == [w[0] for w in full]  # the pass does not depend on capacity
        if cap == lo - 3:
            assert (count > cap).all() and (starts >= 0).all()  # the stored prefix, no -1 fill
            assert all(np.array_equal(starts[r], full[r][1][:cap]) for r in range(2))
        elif cap > lo:
            assert all((starts[r, count[r]:] == -1).all() and (starts[r, :count[r]] >= 0).all() for r in range(2))
    # out=: written in place, every slot of it
    cap = lo + 2
    out = amd.stream.FoundFrames(count=torch.full((2,), 99, dtype=torch.int32, device="cuda"),
                                 starts=torch.full((2, cap), 99, dtype=torch.int64, device="cuda"),
                                 end=torch.full((2,), 99, dtype=torch.int64, device="cuda"))
    got = amd.stream.find_frames_device(met, hop, sf, osr, fs, capacity=cap, out=out)
    assert got is out
    check(out, [expected(m, hop, sf, osr, fs, 0.0, 0, None, capacity=cap) for m in ms])
    with pytest.raises(ValueError):
        amd.stream.find_frames_device(met, hop, sf, osr, fs, capacity=cap + 1, out=out)
    with pytest.raises(TypeError):
        bad = amd.stream.FoundFrames(out.count.to(torch.int64), out.starts, out.end)
        amd.stream.find_frames_device(met, hop, sf, osr, fs, capacity=cap, out=bad)


def test_a_second_sync_word(amd):
    sf, osr, k, W, frac, fs = cases()[0]
    hop = (1 << sf) * osr // k
    m = synthetic(400, sf, k, W, frac, 0x34)
    want = expected(m, hop, sf, osr, fs, 0.0, 0, None, sync=0x34)
    assert want[0] > 100
    check(amd.stream.find_frames_device(to_device(amd, [m]), hop, sf, osr, fs, sync=0x34), [want])


# ---- agreement with the existing finder ------------------------------------------------------

FIELDS = ("symbols", "sync", "cfo", "time_offset", "max_amp")


def same_result(got, keep, want):
    """The slots `keep` (bool [F]) of DemodResult `got` equal DemodResult `want` bit for bit."""
    keep = torch.as_tensor(keep).reshape(-1).cpu().numpy().astype(bool)
    for name in FIELDS:
        a, b = getattr(got, name).cpu().numpy()[keep], getattr(want, name).cpu().numpy()
        assert a.shape == b.shape and a.dtype == b.dtype, name
        if a.dtype == np.float32:
            a, b = dc.bits(a), dc.bits(b)
        assert np.array_equal(a, b), name


@functools.lru_cache(maxsize=None)
def table_stream(ci):
    from oracle.pyoracle import Oracle

    sf, osr, k, S, gaps, sigma, sync = sc.TABLE[ci]
    return sc.planted_stream(Oracle(), sf, osr, S, gaps, sigma, sync, sc.table_seed(ci))


@pytest.mark.parametrize("ci", range(len(sc.TABLE)))
def test_receive_device_equals_receive(amd, ci):
    sf, osr, k, S, gaps, sigma, sync = sc.TABLE[ci]
    hop = (1 << sf) * osr // k
    x, planted, syms = table_stream(ci)
    xd = torch.from_numpy(x).cuda()
    plan = amd.DemodPlan(sf, osr, dechirp=True)
    starts, res = amd.stream.receive(plan, xd, S, hop=hop, sync=sync)
    got = amd.stream.receive_device(plan, xd, S, hop=hop, sync=sync)
    torch.cuda.synchronize()
    cap = len(x) // ((S + 2) * (1 << sf) * osr)
    assert got.found.starts.shape == (1, cap) and got.result.symbols.shape == (cap, S)
    valid = got.found.valid
    assert int(got.found.count[0]) == len(planted)
    assert got.found.starts[valid].cpu().tolist() == starts.cpu().tolist() == planted.tolist()
    assert (got.found.starts[~valid] == -1).all()
    assert int(got.found.end[0]) == planted[-1] + (S + 2) * (1 << sf) * osr
    same_result(got.result, valid, res)
    assert np.array_equal(got.result.symbols.cpu().numpy()[valid[0].cpu().numpy()] % (1 << sf), syms)


GROUPS = sorted({(t[0], t[1]) for t in sc.TABLE})


@pytest.mark.parametrize("sf,osr", GROUPS)
def test_receive_device_on_a_batch_of_rows(amd, sf, osr):
    """All TABLE rows of one SF and osr as one [R, L] batch, padded with silence to a common
    length, run once with each (hop, sync) the group's rows were planted for: every row equals
    `receive` on that row alone, and a row planted for these parameters returns its frames."""
    rows = [ci for ci, t in enumerate(sc.TABLE) if (t[0], t[1]) == (sf, osr)]
    S = sc.TABLE[rows[0]][3]
    assert all(sc.TABLE[ci][3] == S for ci in rows)
    step = (1 << sf) * osr
    L = max(len(table_stream(ci)[0]) for ci in rows) + 3
    x = np.zeros((len(rows), L), np.complex64)
    for r, ci in enumerate(rows):
        x[r, :len(table_stream(ci)[0])] = table_stream(ci)[0]
    xd = torch.from_numpy(x).cuda()
    plan = amd.DemodPlan(sf, osr, dechirp=True)
    cap = L // ((S + 2) * step)
    for k, sync in sorted({(sc.TABLE[ci][2], sc.TABLE[ci][6]) for ci in rows}):
        hop = step // k
        got = amd.stream.receive_device(plan, xd, S, hop=hop, sync=sync)
        torch.cuda.synchronize()
        assert got.found.starts.shape == (len(rows), cap) and got.result.symbols.shape == (len(rows) * cap, S)
        valid = got.found.valid
        for r, ci in enumerate(rows):
            starts, res = amd.stream.receive(plan, xd[r], S, hop=hop, sync=sync)
            assert int(got.found.count[r]) == len(starts)
            assert got.found.starts[r][valid[r]].cpu().tolist() == starts.cpu().tolist()
            keep = torch.zeros_like(valid)
            keep[r] = valid[r]
            same_result(got.result, keep, res)
            if (sc.TABLE[ci][2], sc.TABLE[ci][6]) == (k, sync):
                assert starts.cpu().tolist() == table_stream(ci)[1].tolist()
                assert np.array_equal(res.symbols.cpu().numpy() % (1 << sf), table_stream(ci)[2])


def test_short_rows_and_refusals(amd):
    plan = amd.DemodPlan(7, dechirp=True)
    x = torch.zeros((2, 4000), dtype=torch.complex64, device="cuda")
    got = amd.stream.receive_device(plan, x, 6)  # silence: nothing found, three slots demodulated
    torch.cuda.synchronize()
    assert got.found.count.cpu().tolist() == [0, 0] and got.found.end.cpu().tolist() == [0, 0]
    assert got.found.starts.shape == (2, 3) and (got.found.starts == -1).all() and got.result.symbols.shape == (6, 6)
    plan2 = amd.DemodPlan(7, dechirp=True)
    for L in (1000, 100, 0):  # shorter than a frame, than a window, empty: capacity 0 and no demod call
        got = amd.stream.receive_device(plan2, x[:, :L], 6, first=5)
        torch.cuda.synchronize()
        assert got.found.starts.shape == (2, 0) and got.found.count.cpu().tolist() == [0, 0]
        assert got.found.end.cpu().tolist() == [5, 5]
        assert got.result.symbols.shape == (0, 6) and got.result.sync.shape == (0,)
    assert plan2.last_kernels() == set()  # run() never ran on this plan
    with pytest.raises(ValueError):
        amd.stream.receive_device(amd.DemodPlan(7), x, 6)  # a plan that does not dechirp
    with pytest.raises(ValueError):
        amd.stream.receive_device(plan, x, 6, hop=48)
    with pytest.raises(ValueError):
        amd.stream.receive_device(amd.DemodPlan(7, bw=250000, dechirp=True), x, 6)
    with pytest.raises(ValueError):
        amd.stream.receive_device(plan, x, 6, first=torch.zeros(3, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        amd.stream.receive_device(plan, x[:, :1000], 6, capacity=2)  # no frame fits such a row


# ---- wideband --------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def wideband_case(kind):
    """(sf, osr, S, Channelizer arguments, stream as numpy, scale): channel_checker's end-to-end
    configuration 0 (all channels, sigma 0.1), and resample_checker.CONFIGS[0] as complex64 and
    as cs16 - quantised at four times the default scale, since its two full-scale channels sum to
    more than 1."""
    from oracle.pyoracle import Oracle

    if kind == "integer":
        sf, osr, D, period, T, cutoff, rows, steps, amps = cc.CONFIGS[0]
        x, planted, taps = cc.config_signal(Oracle(), 0, 0, 0.1)
        return sf, osr, planted[0][1].shape[1], (D, taps, period, steps, 1), x, None
    sf, osr, Li, D, period, T, rows, steps, amps = rc.CONFIGS[0]
    x, planted, taps = rc.config_signal(Oracle(), 0, 0.0 if kind == "cs16" else 0.1)
    if kind == "cs16":
        from lora_phy_amd import iq_io

        scale = 4.0 / 32768.0
        assert np.abs(x.real).max() < 4.0 and np.abs(x.imag).max() < 4.0  # nothing clips
        x = iq_io.quantize(torch.from_numpy(x), torch.int16, scale).numpy()
        return sf, osr, planted[0][1].shape[1], (D, taps, period, steps, Li), x, scale
    return sf, osr, planted[0][1].shape[1], (D, taps, period, steps, Li), x, None


@pytest.mark.parametrize("kind", ["integer", "rational", "cs16"])
def test_receive_wideband_device_equals_receive_wideband(amd, kind):
    sf, osr, S, (D, taps, period, steps, Li), x, scale = wideband_case(kind)
    plan = amd.DemodPlan(sf, osr, dechirp=True)
    chan = amd.stream.Channelizer(D, taps, period, steps, interp=Li)
    xd = torch.from_numpy(x).cuda()
    ch, st, res = amd.stream.receive_wideband(plan, chan, xd, S, scale=scale)
    got = amd.stream.receive_wideband_device(plan, chan, xd, S, scale=scale)
    torch.cuda.synchronize()
    assert len(st) >= len(steps)  # every channel carries a frame
    C, Wc = chan.run(xd, scale=scale).shape
    cap = Wc // ((S + 2) * (1 << sf) * osr)
    assert got.found.starts.shape == (C, cap) and got.result.symbols.shape == (C * cap, S)
    valid = got.found.valid
    channel = torch.arange(C, device="cuda")[:, None].expand(C, cap)
    assert channel[valid].cpu().tolist() == ch.cpu().tolist()
    assert got.found.starts[valid].cpu().tolist() == st.cpu().tolist()
    assert got.found.count.cpu().tolist() == [int((ch == c).sum()) for c in range(C)]
    same_result(got.result, valid, res)
    # the block forms
    demod = amd.LoRaDemod(sf, mtu=4, osr=osr)
    b_ch, b_st, b_syms = demod.work_wideband(chan, xd, S, scale=scale)
    found, syms = demod.work_wideband_device(chan, xd, S, scale=scale)
    torch.cuda.synchronize()
    assert syms.shape == (C, cap, 4) and demod.last.symbols.shape == (C * cap, S)
    assert found.starts[found.valid].cpu().tolist() == b_st.cpu().tolist()
    keep = found.valid.cpu()  # (torch indexes no uint16 tensor on the device)
    assert torch.equal(syms.cpu()[keep], b_syms.cpu())
    assert torch.equal(demod.last.symbols.cpu()[keep.reshape(-1)], res.symbols.cpu())


def test_work_stream_device_equals_work_stream(amd):
    sf, osr, k, S, gaps, sigma, sync = sc.TABLE[1]
    x, planted, want = table_stream(1)
    xd = torch.from_numpy(x).cuda()
    demod = amd.LoRaDemod(sf, mtu=4)
    starts, syms = demod.work_stream(xd, S)
    last = demod.last
    found, got = demod.work_stream_device(xd, S)
    torch.cuda.synchronize()
    assert got.shape == (1, found.starts.shape[1], 4)
    assert found.starts[found.valid].cpu().tolist() == starts.cpu().tolist() == planted.tolist()
    assert torch.equal(got.cpu()[found.valid.cpu()], syms.cpu()) and np.array_equal(syms.cpu().numpy(), want[:, :4])
    same_result(demod.last, found.valid, last)


# ---- chunks, and no synchronisation ----------------------------------------------------------

class no_sync:
    """torch's synchronisation debug mode at "error", restored on the way out."""

    def __enter__(self):
        self.prev = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")

    def __exit__(self, *exc):
        torch.cuda.set_sync_debug_mode(self.prev)
        return False


def test_two_chunks_carry_end_on_the_device(amd):
    """TABLE[1]'s stream (frames at 37, 1066, 2391 and 4315, 1024 samples each) in two chunks: the
    second begins at sample 1500, inside the second frame, and the first ends at 2524, inside the
    third.  A chunk keeps every frame that lies wholly inside it; the next chunk's `first` is the
    previous `end` minus the advance, clamped at 0 - a tensor operation, so both chunks are
    enqueued before anything is read back (the synchronisation debug mode would raise)."""
    sf, osr, k, S, gaps, sigma, sync = sc.TABLE[1]
    x, planted, syms = table_stream(1)
    frame_len = (S + 2) * (1 << sf)
    advance = 1500
    assert any(s < advance < s + frame_len for s in planted) and any(s < advance + frame_len < s + frame_len
                                                                     for s in planted)
    xd = torch.from_numpy(x).cuda()
    plan = amd.DemodPlan(sf, dechirp=True)
    starts, res = amd.stream.receive(plan, xd, S)
    a_in, b_in = xd[:advance + frame_len], xd[advance:]
    amd.stream.receive_device(plan, a_in, S)  # (warm-up: the plan's workspace is allocated here)
    torch.cuda.synchronize()
    with no_sync():
        a = amd.stream.receive_device(plan, a_in, S)
        b = amd.stream.receive_device(plan, b_in, S, first=(a.found.end - advance).clamp_min(0))
    torch.cuda.synchronize()
    got = torch.cat([a.found.starts[a.found.valid], b.found.starts[b.found.valid] + advance])
    assert got.cpu().tolist() == starts.cpu().tolist() == planted.tolist()
    assert int(a.found.count[0]) == 2 and int(b.found.count[0]) == 2
    assert int(b.found.end[0]) + advance == planted[-1] + frame_len
    ka, kb = a.found.valid[0].cpu(), b.found.valid[0].cpu()  # (torch indexes no uint16 tensor on the device)
    both = amd.DemodResult(*(torch.cat([getattr(a.result, n).cpu()[ka], getattr(b.result, n).cpu()[kb]]) for n in FIELDS))
    same_result(both, torch.ones(len(planted), dtype=torch.bool), res)


def test_the_device_calls_do_not_synchronise(amd):
    sf, osr, k, S, gaps, sigma, sync = sc.TABLE[1]
    xd = torch.from_numpy(table_stream(1)[0]).cuda()
    plan = amd.DemodPlan(sf, dechirp=True)
    wsf, wosr, wS, (D, taps, period, steps, Li), wx, _ = wideband_case("integer")
    wplan = amd.DemodPlan(wsf, wosr, dechirp=True)
    chan = amd.stream.Channelizer(D, taps, period, steps, interp=Li)
    wxd = torch.from_numpy(wx).cuda()
    hop = plan.step // 4
    met = plan.scan(xd, hop)
    first = torch.zeros(1, dtype=torch.int64, device="cuda")
    # once outside the mode, so that the plans' workspaces exist
    want = amd.stream.receive_device(plan, xd, S)
    wwant = amd.stream.receive_wideband_device(wplan, chan, wxd, wS)
    torch.cuda.synchronize()
    with no_sync():
        # the mode detects what it should on this build: the host finder's copy raises
        with pytest.raises(RuntimeError):
            amd.stream.receive(plan, xd, S)
        found = amd.stream.find_frames_device(met, hop, sf, osr, S, first=first, row_len=xd.shape[0])
        found2 = amd.stream.find_frames_device(met, hop, sf, osr, S, first=3, row_len=xd.shape[0])
        got = amd.stream.receive_device(plan, xd, S, first=first)
        wgot = amd.stream.receive_wideband_device(wplan, chan, wxd, wS)
    torch.cuda.synchronize()
    assert torch.equal(found.starts, want.found.starts) and torch.equal(found2.count, want.found.count)
    assert torch.equal(got.found.starts, want.found.starts) and torch.equal(got.result.symbols, want.result.symbols)
    assert torch.equal(wgot.found.starts, wwant.found.starts)
    assert torch.equal(wgot.result.symbols, wwant.result.symbols)
