"""GPU: receiving self-describing frames from a stream on soft decisions
(stream.receive_frames_device / receive_wideband_frames_device / LoRaDemod.work_packets_device
with soft=True).

As in tests/test_gpu_frames_stream.py, expected values never come from the new code: the whole
chain is compared with the same chain on the CPU (frame_soft_checker.receive_frames_soft_host:
the oracle's scan, demodulator and windows, the checker's soft header gate, pass and soft
decode), after that host chain has been shown to return every planted frame."""
import functools

import numpy as np
import pytest

from tests import channel_checker as cc
from tests import detect_checker as dc
from tests import frame_checker as fc
from tests import frame_soft_checker as fs
from tests import soft_checker as sc
from tests.test_gpu_frames_stream import SYNC, dev, fc_capacity, no_sync, padded, planted, same_chain

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

# the shapes of tests/test_gpu_frames_stream.py's chain test at SF 7 and 9: (sf, osr, k, sigma)
E2E = [(7, 1, 4, 0.0), (7, 1, 4, 0.1), (7, 2, 2, 0.0), (7, 2, 2, 0.02), (9, 1, 2, 0.0), (9, 1, 2, 0.1),
       (9, 2, 4, 0.0), (9, 2, 4, 0.02)]
MAX_SYMBOLS = 40


@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import lora_phy_amd

    return lora_phy_amd


@functools.lru_cache(maxsize=None)
def oracle():
    from oracle.pyoracle import Oracle

    return Oracle()


def same_soft_chain(got, host, sf):
    """A one-row StreamPackets of soft=True against receive_frames_soft_host's result."""
    K = len(host["starts"])
    cap = got.found.starts.shape[1]
    assert K <= cap
    assert int(got.found.count[0]) == K and int(got.found.end[0]) == host["end"]
    assert int(got.candidates[0]) == len(host["candidates"])
    assert np.array_equal(got.found.starts[0].cpu().numpy(), padded(host["starts"], cap, -1, np.int64))
    assert np.array_equal(got.nsym[0].cpu().numpy(), padded(host["nsym"], cap, 0, np.int32))
    fr = got.frames
    for name, key in (("status", "status"), ("nbytes", "nbytes"), ("rdd", "rdd"), ("has_crc", "crc"),
                      ("nsym", "nsym"), ("errors", "errors"), ("hdr_flips", "hdr_flips")):
        assert getattr(fr, name).cpu().numpy()[:K].tolist() == [f[key] for f in host["frames"]], name
    pay = fr.payload.cpu().numpy()
    llr = got.llr.cpu().numpy()
    assert got.llr.shape == (cap, 2 + MAX_SYMBOLS, sf)
    for j, f in enumerate(host["frames"]):
        assert np.array_equal(pay[j], f["payload"]), j
        assert np.array_equal(dc.bits(llr[j]), dc.bits(f["llr"])), j  # the slot's soft bits, bit for bit
        sym = got.result.symbols[j].cpu().numpy()
        assert np.array_equal(sym[:len(f["symbols"])], f["symbols"]), j


@pytest.mark.parametrize("sf,osr,k,sigma", E2E)
def test_soft_chain_equals_the_host_chain(amd, sf, osr, k, sigma):
    x, starts, pays, nsym = planted(sf, osr, sigma)
    max_bytes = fc_capacity(sf, MAX_SYMBOLS)
    hop = (1 << sf) * osr // k
    host = fs.receive_frames_soft_host(oracle(), x, sf, osr, MAX_SYMBOLS, hop, SYNC, 0.0, max_bytes=max_bytes)
    # the condition on the inputs: the host chain returns every planted frame
    assert host["starts"].tolist() == starts and host["nsym"].tolist() == nsym
    for f, pay in zip(host["frames"], pays):
        assert f["status"] == fc.OK and f["payload"][:len(pay)].tobytes() == pay and f["nbytes"] == len(pay)
    plan = amd.DemodPlan(sf, osr, dechirp=True)
    xd = dev(x, np.complex64)
    amd.stream.receive_frames_device(plan, xd, MAX_SYMBOLS, hop=hop, soft=True)  # (workspaces exist after this)
    torch.cuda.synchronize()
    with no_sync():
        got = amd.stream.receive_frames_device(plan, xd, MAX_SYMBOLS, hop=hop, soft=True)
    torch.cuda.synchronize()
    same_soft_chain(got, host, sf)


def test_soft_false_is_the_hard_chain_field_by_field(amd):
    sf, osr, k, sigma = 7, 1, 4, 0.1
    x = planted(sf, osr, sigma)[0]
    plan = amd.DemodPlan(sf, osr, dechirp=True)
    xd = dev(x, np.complex64)
    host = fc.receive_frames_host(oracle(), x, sf, osr, MAX_SYMBOLS, plan.step // k, SYNC, 0.0,
                                  max_bytes=fc_capacity(sf, MAX_SYMBOLS))
    for kw in ({}, {"soft": False}, {"soft": False, "max_flips": 0}):
        got = amd.stream.receive_frames_device(plan, xd, MAX_SYMBOLS, hop=plan.step // k, **kw)
        torch.cuda.synchronize()
        same_chain(amd, got, host, plan, sf)
        assert got.llr is None and got.frames.hdr_flips is None
    # the block form, both ways
    demod = amd.LoRaDemod(sf, mtu=MAX_SYMBOLS)
    soft = amd.stream.receive_frames_device(plan, xd, MAX_SYMBOLS, soft=True, max_flips=3)
    pk = demod.work_packets_device(xd, soft=True, max_flips=3)
    torch.cuda.synchronize()
    assert torch.equal(pk.frames.payload, soft.frames.payload) and torch.equal(pk.frames.hdr_flips, soft.frames.hdr_flips)
    assert torch.equal(pk.llr, soft.llr) and demod.last is pk.result
    hard = demod.work_packets_device(xd)
    assert hard.llr is None and torch.equal(hard.frames.payload, got.frames.payload)
    with pytest.raises(ValueError):
        amd.stream.receive_frames_device(plan, xd, MAX_SYMBOLS, soft=True, max_flips=41)


# One row the hard chain loses a frame of and the soft chain does not: three frames of 14, 14 and 9
# bytes at CR 4/5 with the CRC, SF 7, white noise of soft_checker.noise_sigma(WEAK_DB) per component
# drawn from default_rng(WEAK_SEED) after the payloads, the finder at thresh_db = -14 (at 0 dB it
# lists nothing in this noise).  The seed was chosen on the CPU with the two host chains: the first
# of 1, 2, ... at which the hard chain returns status CRC for a planted frame that the soft chain
# returns OK with its payload (seed 1: the frame at sample 40; seeds 6 and 11 do the same).
WEAK_DB, WEAK_SEED, WEAK_THRESH = -5.0, 1, -14.0
WEAK_SPECS, WEAK_GAPS = ((14, 1, 1), (14, 1, 1), (9, 1, 1)), (40, 300, 17)


@functools.lru_cache(maxsize=None)
def weak_row():
    O = oracle()
    sf = 7
    rng = np.random.default_rng(WEAK_SEED)
    parts, starts, pays, at = [], [], [], 0
    for (n, rdd, crc), g in zip(WEAK_SPECS, WEAK_GAPS):
        pay = rng.integers(0, 256, n).astype(np.uint8).tobytes()
        iq = O.lora_modulate(fc.encode_frame(pay, sf, rdd, crc), sf, 1, 125000, 1.0, SYNC)
        parts += [np.zeros(g, np.complex64), iq]
        starts.append(at + g)
        at += g + len(iq)
        pays.append(pay)
    x = np.concatenate(parts + [np.zeros(50, np.complex64)])
    s = sc.noise_sigma(WEAK_DB)
    x = (x + s * (rng.standard_normal(len(x)) + 1j * rng.standard_normal(len(x)))).astype(np.complex64)
    return x, starts, pays


def test_soft_returns_a_frame_the_hard_chain_fails(amd):
    sf, k = 7, 4
    x, starts, pays = weak_row()
    O = oracle()
    hard_host = fc.receive_frames_host(O, x, sf, 1, MAX_SYMBOLS, 128 // k, SYNC, WEAK_THRESH,
                                         max_bytes=fc_capacity(sf, MAX_SYMBOLS))
    soft_host = fs.receive_frames_soft_host(O, x, sf, 1, MAX_SYMBOLS, 128 // k, SYNC, WEAK_THRESH,
                                         max_bytes=fc_capacity(sf, MAX_SYMBOLS))
    plan = amd.DemodPlan(sf, dechirp=True)
    xd = dev(x, np.complex64)
    hard = amd.stream.receive_frames_device(plan, xd, MAX_SYMBOLS, thresh_db=WEAK_THRESH)
    soft = amd.stream.receive_frames_device(plan, xd, MAX_SYMBOLS, thresh_db=WEAK_THRESH, soft=True)
    torch.cuda.synchronize()
    same_chain(amd, hard, hard_host, plan, sf)
    same_soft_chain(soft, soft_host, sf)
    hs = dict(zip(hard.found.starts[0].cpu().tolist(), hard.frames.status.cpu().tolist()))
    ss = dict(zip(soft.found.starts[0].cpu().tolist(), range(soft.found.starts.shape[1])))
    mended = [(a, p) for a, p in zip(starts, pays) if hs.get(a) == fc.CRC and a in ss
              and int(soft.frames.status[ss[a]]) == fc.OK]
    assert mended, (hs, soft.frames.status.cpu().tolist())
    for a, p in mended:
        j = ss[a]
        assert bytes(soft.frames.payload[j].cpu().numpy()[:len(p)]) == p and int(soft.frames.errors[j]) > 0


def test_wideband_soft_chain_through_the_channelizer(amd):
    """LoRaMod.work_frame -> transmit_wideband -> noise -> receive_wideband_frames_device(soft=True):
    the channel rows the bank gives are received on the host, row by row, by the soft host chain,
    which returns every planted frame; the device chain equals it."""
    sf, osr, D, period, T, cutoff = cc.CONFIGS[0][:6]
    steps = (-1, 1)
    step = (1 << sf) * osr
    rng = np.random.default_rng(8)
    pay = rng.integers(0, 256, (4, 16)).astype(np.uint8)
    nbytes = np.array([0, 12, 5, 16])
    channel = np.array([0, 0, 1, 1])
    frames = amd.LoRaMod(sf, ovs=osr, cr=1).work_frame(pay, nbytes)
    nsym = np.array([fc.frame_symbols(sf, n, 1, 1) for n in nbytes])
    S = int(nsym.max())
    starts = np.array([64, 64 + 15 * step + 40, 200, 200 + 20 * step + 3])
    chan_len = int(starts.max()) + (2 + S) * step + 64
    syn = amd.stream.Synthesizer(D, amd.stream.lowpass_taps(T, 0.5 / D, gain=D), period, steps)
    x = None
    for f in range(4):
        part = amd.stream.transmit_wideband(syn, frames[f:f + 1, :(2 + int(nsym[f])) * step], [int(channel[f])],
                                            [int(starts[f])], chan_len)
        x = part if x is None else x + part
    noise = 0.05 * (rng.standard_normal(x.shape[0]) + 1j * rng.standard_normal(x.shape[0]))
    x = x + torch.from_numpy(noise.astype(np.complex64)).cuda()
    plan = amd.DemodPlan(sf, osr, dechirp=True)
    chan = amd.stream.Channelizer(D, amd.stream.lowpass_taps(T, cutoff), period, steps)
    got = amd.stream.receive_wideband_frames_device(plan, chan, x, S, soft=True)
    rows = chan.run(x).cpu().numpy()
    torch.cuda.synchronize()
    cap = got.found.starts.shape[1]
    max_bytes = fc_capacity(sf, S)
    for r in range(2):
        host = fs.receive_frames_soft_host(oracle(), rows[r], sf, osr, S, plan.step // 4, SYNC, 0.0, max_bytes=max_bytes)
        assert len(host["frames"]) == 2
        for f, j in zip(host["frames"], np.flatnonzero(channel == r)):
            assert f["status"] == fc.OK and f["nbytes"] == nbytes[j]
            assert np.array_equal(f["payload"][:nbytes[j]], pay[j, :nbytes[j]])
        assert int(got.found.count[r]) == 2
        assert got.found.starts[r, :2].cpu().tolist() == host["starts"].tolist()
        for i, f in enumerate(host["frames"]):
            slot = r * cap + i
            for name, key in (("status", "status"), ("nbytes", "nbytes"), ("rdd", "rdd"), ("has_crc", "crc"),
                              ("nsym", "nsym"), ("errors", "errors"), ("hdr_flips", "hdr_flips")):
                assert int(getattr(got.frames, name)[slot]) == f[key], (r, i, name)
            assert np.array_equal(got.frames.payload[slot].cpu().numpy(), f["payload"]), (r, i)
            assert np.array_equal(dc.bits(got.llr[slot].cpu().numpy()), dc.bits(f["llr"][:2 + S])), (r, i)


def test_sweep_receives_the_same_rows_both_ways(amd):
    """awgn.sweep_receive_frames(soft=): the same seeded rows, hard and soft; at +10 dB both return
    every planted frame, and the records say which way they were received."""
    from lora_phy_amd import awgn

    kw = dict(frames=16, max_bytes=12, cr=1, seed=5)
    hard = awgn.sweep_receive_frames(7, [10.0], **kw)[0]
    soft = awgn.sweep_receive_frames(7, [10.0], soft=True, **kw)[0]
    assert "soft" not in hard and soft["soft"] is True and soft["max_flips"] == 5
    assert hard["planted"] == soft["planted"] == 16 and hard["returned_ok"] == soft["returned_ok"] == 16
    assert hard["candidates"] == soft["candidates"] and soft["false_frames"] == 0
