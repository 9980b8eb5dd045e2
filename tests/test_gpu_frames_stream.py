"""GPU: receiving self-describing frames from a stream with no frame length given
(lora_phy_amd.stream: find_candidates_device, select_frames_device, receive_frames_device,
receive_wideband_frames_device; LoRaDemod.work_packets_device).

Expected values never come from the new code.  The candidate list and the pass are compared
with their numpy restatements (tests/frame_checker.py) on synthetic metrics, integer for integer;
the whole chain is compared with the same chain on the CPU (frame_checker.receive_frames_host:
the oracle's scan and demodulator, the checker's header gate, pass and decode), after that host
chain has been shown to return every planted frame."""
import functools

import numpy as np
import pytest

from tests import channel_checker as cc
from tests import frame_checker as fc
from tests import synth_checker as sy

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SYNC = 0x12


@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import lora_phy_amd

    return lora_phy_amd


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def padded(a, n, fill, dtype):
    return fc.to_slots(a, n, fill, dtype)


class no_sync:
    """torch's synchronisation debug mode at "error", restored on the way out."""

    def __enter__(self):
        self.prev = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")

    def __exit__(self, *exc):
        torch.cuda.set_sync_debug_mode(self.prev)
        return False


# ---- the candidate list and the pass, on synthetic metrics ------------------------------------

def scan_cases():
    """(sf, osr, k, W, frac): W below one turn of the candidate kernel (1024 windows), across
    several, below and above the finder's tile, and a scan with fewer windows than k."""
    from lora_phy_amd import _capi

    tile = _capi.FIND_TILE
    return [(7, 1, 4, 700, 0.3), (7, 1, 4, 1024 + 4, 0.5), (9, 2, 8, tile - 5, 0.2), (12, 1, 2, tile + 37, 0.3),
            (7, 2, 4, 2 * tile + 1029, 0.6), (8, 1, 4, 3, 0.5)]


def to_device(amd, ms, stride):
    W = len(ms[0]["index"])

    def put(key, fill):
        buf = np.full((len(ms), stride), fill, ms[0][key].dtype)
        for r, m in enumerate(ms):
            buf[r, :W] = m[key]
        return torch.from_numpy(buf).cuda()[:, :W]

    # what lies between the rows would pass every test if it were read: +inf power, peak sw0
    return amd.DetectMetrics(put("power", np.inf), put("power_avg", 0), None, put("index", 0))


@pytest.mark.parametrize("ci", range(6))
def test_candidates_equal_the_host_model(amd, ci):
    sf, osr, k, W, frac = scan_cases()[ci]
    step = (1 << sf) * osr
    hop = step // k
    ms = [fc.synthetic_scan(10 * ci + r, sf, k, W, frac) for r in range(3)]
    met = to_device(amd, ms, W + 7)
    for row_len, thresh in ((None, 0.0), (max((W - 1) * hop - 3 * hop, 0), 1.5)):
        want = [fc.find_candidates_host(m, hop, sf, osr, SYNC, thresh, row_len) for m in ms]
        most = max(len(w) for w in want)
        if W > 1000:
            assert min(len(w) for w in want) > 20
        for cap in sorted({None, 0, most // 2, most, most + 3}, key=lambda c: -1 if c is None else c):
            count, starts = amd.stream.find_candidates_device(met, hop, sf, osr, SYNC, thresh, row_len, cap)
            rl = ((W - 1) * hop + step if W else 0) if row_len is None else row_len
            C = -(-rl // (4 * step)) if cap is None else cap
            assert count.dtype == torch.int32 and starts.dtype == torch.int64 and starts.shape == (3, C)
            assert count.cpu().tolist() == [len(w) for w in want], (ci, cap)
            got = starts.cpu().numpy()
            for r in range(3):
                assert np.array_equal(got[r], padded(want[r], C, -1, np.int64)), (ci, cap, r)
    one, s1 = amd.stream.find_candidates_device(
        amd.DetectMetrics(met.power[0], met.power_avg[0], None, met.index[0]), hop, sf, osr)
    assert one.shape == (1,) and int(one[0]) == len(fc.find_candidates_host(ms[0], hop, sf, osr))


def test_all_nan_power_lists_nothing(amd):
    sf, osr, k, W = 7, 1, 4, 2100
    m = dict(fc.synthetic_scan(1, sf, k, W, 0.9))
    m["power"] = np.full(W, np.nan, np.float32)
    count, starts = amd.stream.find_candidates_device(to_device(amd, [m], W), 32, sf, osr, cand_capacity=9)
    assert int(count[0]) == 0 and (starts.cpu().numpy() == -1).all() and starts.shape == (1, 9)


@pytest.mark.parametrize("C", [0, 1, 255, 256, 257, 1500])
def test_selection_equals_the_host_model(amd, C):
    """Random slot lists, four rows with a `first` each: starts that mostly grow (candidates come
    in window order) with equal and falling ones among them, every status, frames of 8 to 50
    symbols with max_symbols 40, empty slots; slot counts on both sides of the kernel's 256-slot
    turn; capacities below, at and above the counts, and 0."""
    R, step, max_symbols = 4, 128, 40
    rng = np.random.default_rng(C)
    row_len = 10 * step * max(C, 4)
    starts = np.sort(rng.integers(0, row_len, (R, C)), axis=1) + rng.integers(-300, 300, (R, C))
    starts[rng.random((R, C)) < 0.05] = -1
    status = rng.choice([fc.OK, fc.OK, fc.OK, fc.HEADER, fc.SHORT, fc.CRC], (R, C)).astype(np.int32)
    nsym = rng.integers(8, 51, (R, C)).astype(np.int32)
    first = np.array([0, 1000, row_len // 2, row_len + 5])
    want = [fc.select_frames_host(starts[r], status[r], nsym[r], step, row_len, max_symbols, int(first[r]))
            for r in range(R)]
    most = max(len(w[0]) for w in want)
    if C >= 255:
        assert most > 10 and len(want[3][0]) == 0
    d = [dev(starts, np.int64), dev(status, np.int32), dev(nsym, np.int32)]
    for cap in sorted({None, 0, most // 2, most, most + 3}, key=lambda c: -1 if c is None else c):
        found, got_n = amd.stream.select_frames_device(*d, step, row_len, max_symbols, dev(first, np.int64), cap)
        K = row_len // (10 * step) if cap is None else cap
        assert found.starts.shape == got_n.shape == (R, K) and got_n.dtype == torch.int32
        assert found.count.cpu().tolist() == [len(w[0]) for w in want], (C, cap)
        assert found.end.cpu().tolist() == [w[2] for w in want], (C, cap)
        for r in range(R):
            assert np.array_equal(found.starts[r].cpu().numpy(), padded(want[r][0], K, -1, np.int64)), (C, cap, r)
            assert np.array_equal(got_n[r].cpu().numpy(), padded(want[r][1], K, 0, np.int32)), (C, cap, r)
    # first as None and as an int
    for f in (None, 700):
        found, _ = amd.stream.select_frames_device(*d, step, row_len, max_symbols, f)
        w = [fc.select_frames_host(starts[r], status[r], nsym[r], step, row_len, max_symbols, f or 0)
             for r in range(R)]
        assert found.count.cpu().tolist() == [len(x[0]) for x in w] and found.end.cpu().tolist() == [x[2] for x in w]


# ---- end to end -------------------------------------------------------------------------------

# six frames (payload bytes, rdd, crc) after their gaps (multiples of the osr: the finder's
# resolution): back to back and after gaps
SPECS = [(0, 1, 1), (12, 1, 1), (5, 4, 1), (3, 4, 0), (9, 0, 1), (7, 2, 1)]
GAPS = [38, 0, 0, 302, 6, 900]
# (sf, osr, k, sigma): silence and mild noise.  At osr 2 the noise is milder still: the reference's
# time-offset estimate wanders with it (|offset| 0.2 at sigma 0.02 on these streams, above 0.5 at
# 0.05 at SF9, which moves every bin of a frame by one), and the payload, unlike the header, has no
# margin for that - on the host as on the device, which is why the condition on the inputs is checked
# on the host chain first.
E2E = [(7, 1, 4, 0.0), (7, 1, 4, 0.1), (7, 2, 2, 0.0), (7, 2, 2, 0.02), (9, 1, 2, 0.0), (9, 1, 2, 0.1),
       (9, 2, 4, 0.0), (9, 2, 4, 0.02), (12, 1, 2, 0.1)]


@functools.lru_cache(maxsize=None)
def planted(sf, osr, sigma, specs=None, gaps=None, tail=50):
    """(stream, planted starts, payloads, nsym) of oracle-modulated frames in silence or noise."""
    from oracle.pyoracle import Oracle

    O = Oracle()
    specs = (SPECS if sf < 12 else [(0, 4, 1), (5, 2, 1)]) if specs is None else specs
    gaps = (GAPS if sf < 12 else [1000, 4]) if gaps is None else gaps
    rng = np.random.default_rng(1000 * sf + osr)
    parts, starts, pays, nsym, at = [], [], [], [], 0
    for (n, rdd, crc), g in zip(specs, gaps):
        pay = rng.integers(0, 256, n).astype(np.uint8).tobytes()
        sym = fc.encode_frame(pay, sf, rdd, crc)
        iq = O.lora_modulate(sym, sf, osr, 125000, 1.0, SYNC)
        parts += [np.zeros(g, np.complex64), iq]
        starts.append(at + g)
        at += g + len(iq)
        pays.append(pay)
        nsym.append(len(sym))
    x = np.concatenate(parts + [np.zeros(tail, np.complex64)])
    if sigma:
        rng = np.random.default_rng(77)
        x = (x + sigma * (rng.standard_normal(len(x)) + 1j * rng.standard_normal(len(x)))).astype(np.complex64)
    x.setflags(write=False)
    return x, starts, pays, nsym


@functools.lru_cache(maxsize=None)
def host_chain(sf, osr, k, sigma, max_symbols):
    from oracle.pyoracle import Oracle

    x = planted(sf, osr, sigma)[0]
    return fc.receive_frames_host(Oracle(), x, sf, osr, max_symbols, (1 << sf) * osr // k, SYNC, 0.0,
                                  max_bytes=fc_capacity(sf, max_symbols))


def fc_capacity(sf, nsymbols):
    """codec.frame_capacity restated: the most bytes a frame of so many symbols can state."""
    n = 0
    while n < 255 and fc.frame_symbols(sf, n + 1, 0, 0) <= nsymbols:
        n += 1
    return n


def same_chain(amd, got, host, plan, sf):
    """A one-row StreamPackets against receive_frames_host's result."""
    K = len(host["starts"])
    cap = got.found.starts.shape[1]
    assert K <= cap
    assert int(got.found.count[0]) == K and int(got.found.end[0]) == host["end"]
    assert int(got.candidates[0]) == len(host["candidates"])
    assert np.array_equal(got.found.starts[0].cpu().numpy(), padded(host["starts"], cap, -1, np.int64))
    assert np.array_equal(got.nsym[0].cpu().numpy(), padded(host["nsym"], cap, 0, np.int32))
    fr = got.frames
    for name, key in (("status", "status"), ("nbytes", "nbytes"), ("rdd", "rdd"), ("has_crc", "crc"),
                      ("nsym", "nsym"), ("errors", "errors")):
        assert getattr(fr, name).cpu().numpy()[:K].tolist() == [f[key] for f in host["frames"]], name
    pay = fr.payload.cpu().numpy()
    for j, f in enumerate(host["frames"]):
        assert np.array_equal(pay[j], f["payload"]), j
    # every slot's demodulation is plan.run on its frame zero-padded to the cut, bit for bit
    if K:
        want = plan.run(dev(np.stack([f["padded"] for f in host["frames"]]), np.complex64))
        torch.cuda.synchronize()
        for name in ("symbols", "sync", "cfo", "time_offset", "max_amp"):
            a = getattr(got.result, name).cpu().numpy()[:K]
            b = getattr(want, name).cpu().numpy()
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), name
        # and the oracle's demodulation of it
        sym = got.result.symbols.cpu().numpy()
        for j, f in enumerate(host["frames"]):
            assert np.array_equal(sym[j, :len(f["symbols"])], f["symbols"]), j


@pytest.mark.parametrize("sf,osr,k,sigma", E2E)
def test_chain_equals_the_host_chain(amd, sf, osr, k, sigma):
    max_symbols = 40
    x, starts, pays, nsym = planted(sf, osr, sigma)
    host = host_chain(sf, osr, k, sigma, max_symbols)
    # the condition on the inputs: the host chain returns every planted frame
    assert host["starts"].tolist() == starts and host["nsym"].tolist() == nsym
    for f, pay in zip(host["frames"], pays):
        assert f["status"] == fc.OK and f["payload"][:len(pay)].tobytes() == pay and f["nbytes"] == len(pay)
    plan = amd.DemodPlan(sf, osr, dechirp=True)
    got = amd.stream.receive_frames_device(plan, dev(x, np.complex64), max_symbols, hop=plan.step // k)
    torch.cuda.synchronize()
    assert got.frames.payload.shape[1] == fc_capacity(sf, max_symbols) == amd.codec.frame_capacity(sf, max_symbols)
    same_chain(amd, got, host, plan, sf)


def test_mixed_lengths_need_no_frame_symbols(amd):
    """One row holds frames of 13, 18 and 38 data symbols.  receive_device at any one
    frame_symbols cannot return all three (whatever it returns is cut to that length);
    receive_frames_device returns the three with their payloads."""
    sf = 7
    specs, gaps = ((0, 1, 1), (5, 1, 1), (16, 1, 1)), (40, 200, 0)
    x, starts, pays, nsym = planted(sf, 1, 0.05, specs, gaps)
    assert nsym == [13, 18, 38]
    plan = amd.DemodPlan(sf, dechirp=True)
    xd = dev(x, np.complex64)
    for S in (13, 18, 38):
        fixed = amd.stream.receive_device(plan, xd, S)
        torch.cuda.synchronize()
        kept = fixed.found.starts[fixed.found.valid].cpu().tolist()
        # a frame comes back whole when its start is found and the S columns hold all its symbols
        whole = [s for s, n in zip(starts, nsym) if s in kept and n <= S]
        assert 1 <= len(whole) < 3, (S, kept)
    got = amd.stream.receive_frames_device(plan, xd, 38)
    torch.cuda.synchronize()
    assert got.found.starts[got.found.valid].cpu().tolist() == starts
    assert got.nsym[got.found.valid].cpu().tolist() == nsym
    assert got.frames.status.cpu().tolist()[:3] == [fc.OK] * 3
    for j, pay in enumerate(pays):
        assert bytes(got.frames.payload[j].cpu().numpy()[:len(pay)]) == pay and int(got.frames.nbytes[j]) == len(pay)
    # the block form
    demod = amd.LoRaDemod(sf, mtu=38, cr=4)  # the header's coding rate wins over the block's
    pk = demod.work_packets_device(xd)
    torch.cuda.synchronize()
    assert torch.equal(pk.found.starts, got.found.starts) and torch.equal(pk.frames.payload, got.frames.payload)
    assert demod.last is pk.result


def test_two_chunks_carry_end_on_the_device(amd):
    """The SF7 stream in two chunks that overlap by (2 + max_symbols) * step - 1 samples, the next
    chunk's `first` being the previous `end` less the advance - a tensor operation: both chunks
    are enqueued before anything is read back.  Together they return what one call returns."""
    sf, max_symbols = 7, 40
    x, starts, pays, nsym = planted(sf, 1, 0.1)
    plan = amd.DemodPlan(sf, dechirp=True)
    xd = dev(x, np.complex64)
    whole = amd.stream.receive_frames_device(plan, xd, max_symbols)
    overlap = (2 + max_symbols) * plan.step - 1
    advance = starts[3] + 700  # inside the fourth frame
    a_in, b_in = xd[:advance + overlap], xd[advance:]
    amd.stream.receive_frames_device(plan, a_in, max_symbols)  # (warm-up: workspaces are allocated here)
    amd.stream.receive_frames_device(plan, b_in, max_symbols)
    torch.cuda.synchronize()
    with no_sync():
        a = amd.stream.receive_frames_device(plan, a_in, max_symbols)
        b = amd.stream.receive_frames_device(plan, b_in, max_symbols, first=(a.found.end - advance).clamp_min(0))
    torch.cuda.synchronize()
    assert whole.found.starts[whole.found.valid].cpu().tolist() == starts
    got = torch.cat([a.found.starts[a.found.valid], b.found.starts[b.found.valid] + advance])
    assert got.cpu().tolist() == starts
    assert int(a.found.count[0]) + int(b.found.count[0]) == len(starts) and int(b.found.count[0]) >= 1
    assert int(b.found.end[0]) + advance == int(whole.found.end[0])
    ka, kb = a.found.valid[0].cpu(), b.found.valid[0].cpu()
    both = torch.cat([a.frames.payload.cpu()[ka], b.frames.payload.cpu()[kb]])
    assert torch.equal(both, whole.frames.payload.cpu()[whole.found.valid[0].cpu()])
    status = torch.cat([a.frames.status.cpu()[ka], b.frames.status.cpu()[kb]])
    assert status.tolist() == [fc.OK] * len(starts)


def test_the_chain_does_not_synchronise(amd):
    sf, max_symbols = 7, 40
    xd = dev(planted(sf, 1, 0.1)[0], np.complex64)
    plan = amd.DemodPlan(sf, dechirp=True)
    rows = torch.stack([xd, xd.flip(0)])
    first = torch.zeros(2, dtype=torch.int64, device="cuda")
    demod = amd.LoRaDemod(sf, mtu=max_symbols)
    want = amd.stream.receive_frames_device(plan, rows, max_symbols)  # once outside the mode: workspaces exist
    demod.work_packets_device(rows)
    torch.cuda.synchronize()
    with no_sync():
        with pytest.raises(RuntimeError):  # the mode detects what it should on this build
            amd.stream.receive(plan, xd, 13)
        got = amd.stream.receive_frames_device(plan, rows, max_symbols, first=first)
        demod_got = demod.work_packets_device(rows)
    torch.cuda.synchronize()
    assert torch.equal(got.found.starts, want.found.starts) and torch.equal(got.frames.payload, want.frames.payload)
    assert torch.equal(demod_got.found.count, want.found.count)
    assert want.found.count.cpu().tolist()[0] == 6


def test_wideband_loopback_of_two_channels_with_different_frames(amd):
    """LoRaMod.work_frame -> transmit_wideband -> receive_wideband_frames_device: two channels,
    each with two frames of its own lengths; the frames come back in their channels, moved by the
    two banks' delays, with their payloads."""
    sf, osr, D, period, T, cutoff = cc.CONFIGS[0][:6]
    steps = (-1, 1)
    step = (1 << sf) * osr
    max_bytes = 16
    rng = np.random.default_rng(8)
    pay = rng.integers(0, 256, (4, max_bytes)).astype(np.uint8)
    nbytes = np.array([0, 12, 5, 16])
    channel = np.array([0, 0, 1, 1])
    mod = amd.LoRaMod(sf, ovs=osr, cr=1)
    frames = mod.work_frame(pay, nbytes)
    nsym = np.array([fc.frame_symbols(sf, n, 1, 1) for n in nbytes])
    S = int(nsym.max())
    assert frames.shape == (4, (2 + S) * step)
    starts = np.array([64, 64 + 15 * step + 40, 200, 200 + 20 * step + 3])  # a row's silence may overlap the next
    chan_len = int(starts.max()) + (2 + S) * step + 64
    syn = amd.stream.Synthesizer(D, amd.stream.lowpass_taps(T, 0.5 / D, gain=D), period, steps)
    # frames are placed whole rows at a time: cut each to its own length so that neighbours do not overlap
    x = None
    for f in range(4):
        part = amd.stream.transmit_wideband(syn, frames[f:f + 1, :(2 + int(nsym[f])) * step], [int(channel[f])],
                                            [int(starts[f])], chan_len)
        x = part if x is None else x + part
    plan = amd.DemodPlan(sf, osr, dechirp=True)
    chan = amd.stream.Channelizer(D, amd.stream.lowpass_taps(T, cutoff), period, steps)
    got = amd.stream.receive_wideband_frames_device(plan, chan, x, S)
    torch.cuda.synchronize()
    shift = sy.loopback_shift(T, D, T, D)
    assert got.found.count.cpu().tolist() == [2, 2]
    assert got.found.starts[:, :2].cpu().numpy().reshape(-1).tolist() == (starts + shift).tolist()
    assert got.nsym[:, :2].cpu().numpy().reshape(-1).tolist() == nsym.tolist()
    cap = got.found.starts.shape[1]
    status = got.frames.status.view(2, cap)[:, :2].cpu().numpy().reshape(-1)
    assert status.tolist() == [fc.OK] * 4
    payload = got.frames.payload.view(2, cap, -1)[:, :2].cpu().numpy().reshape(4, -1)
    for f, n in enumerate(nbytes):
        assert np.array_equal(payload[f, :n], pay[f, :n]) and not payload[f, n:].any(), f
    pk = amd.LoRaDemod(sf, osr=osr, mtu=S).work_wideband_packets_device(chan, x)
    torch.cuda.synchronize()
    assert torch.equal(pk.found.starts, got.found.starts) and torch.equal(pk.frames.payload, got.frames.payload)


def test_refusals_and_short_rows(amd):
    plan = amd.DemodPlan(7, dechirp=True)
    x = torch.zeros(5000, dtype=torch.complex64, device="cuda")
    with pytest.raises(ValueError):
        amd.stream.receive_frames_device(amd.DemodPlan(6, dechirp=True), x, 40)   # SF6 has no header block
    with pytest.raises(ValueError):
        amd.stream.receive_frames_device(plan, x, 7)                               # shorter than a header
    with pytest.raises(ValueError):
        amd.stream.receive_frames_device(amd.DemodPlan(7), x, 40)                  # no dechirp
    with pytest.raises(ValueError):
        amd.stream.receive_frames_device(plan, x, 40, hop=100)
    # silence, a row shorter than a header, a row shorter than a window: nothing found, all written
    for L in (5000, 1000, 100):
        got = amd.stream.receive_frames_device(plan, x[:L], 40)
        torch.cuda.synchronize()
        assert got.found.count.cpu().tolist() == [0] and got.candidates.cpu().tolist() == [0]
        assert got.found.end.cpu().tolist() == [0] and (got.found.starts.cpu().numpy() == -1).all()
        assert got.found.starts.shape == (1, L // 1280)
    none = amd.stream.receive_frames_device(plan, x, 40, capacity=0)
    assert none.result.symbols.shape == (0, 40) and none.frames.payload.shape[0] == 0


def test_sweep_receive_frames_counts(amd):
    """awgn.sweep_receive_frames on a few rows: at +10 dB every planted frame of the mixed lengths
    comes back with its payload and nothing else does; far below the noise nothing comes back;
    noise alone is counted in a record of its own."""
    from lora_phy_amd import awgn

    recs = awgn.sweep_receive_frames(7, [10.0, -30.0], frames=24, max_bytes=12, cr=2, seed=5,
                                     noise_windows=1000, noise_batch_samples=1 << 18)
    hi, lo, noise = recs
    assert hi["planted"] == lo["planted"] == 24 and hi["max_symbols"] == amd.codec.frame_symbols(7, 2, 12)
    assert hi["returned_ok"] == hi["found_at_planted"] == 24 and hi["p_ok"] == 1.0 and hi["false_frames"] == 0
    assert hi["candidates"] >= 24 and hi["candidates_dropped"] == 0
    assert lo["returned_ok"] == 0 and lo["false_frames_ok"] == 0
    assert noise["noise_only"] and noise["windows"] >= 1000 and noise["false_frames"] == 0
