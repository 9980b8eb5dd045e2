"""GPU: preambled frames through the propagation stage and then the preambled receive chain
(stream.propagate -> stream.receive_preamble_frames_device), noiseless and small.  The device
chain is held to its host model (tests/preamble_checker.receive_host with frame_checker's gate and
decode) on the same propagated rows, as integers: starts, offsets, nsym, status and payloads.

What the host model itself returns on these rows: a whole-sample delay is a slice and every planted frame comes
back; at SF9 osr 1 a quarter of a sample and a second path 1.5 samples late at -6 dB still give
every frame with its exact payload; at SF7 osr 2 half a sample and the two paths give every start
but not every payload, and those cases hold the device to the host model only."""
import numpy as np
import pytest

from tests import frame_checker as fc
from tests import preamble_checker as pc
from tests import propagate_checker as pp

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TWO_PATHS = dict(delay=[0.0, 1.5], gain=[1.0, 0.5j])
# (sf, osr, gaps, propagate's arguments, whole samples the frames move, the host model returns every payload)
CASES = {
    "sf7-osr2-whole": (7, 2, (36, 6, 300), dict(delay=4.0), 4, True),
    "sf7-osr2-half": (7, 2, (36, 6, 300), dict(delay=0.5), 0, False),
    "sf7-osr2-two-paths": (7, 2, (36, 6, 300), TWO_PATHS, 0, False),
    "sf9-osr1-whole": (9, 1, (37, 1301), dict(delay=4.0), 4, True),
    "sf9-osr1-quarter": (9, 1, (37, 1301), dict(delay=0.25), 0, True),
    "sf9-osr1-two-paths": (9, 1, (37, 1301), TWO_PATHS, 0, True),
}


@pytest.fixture(scope="module")
def O():
    from oracle.pyoracle import Oracle

    return Oracle()


@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import lora_phy_amd

    return lora_phy_amd


_streams = {}


def clean_stream(O, sf, osr, gaps):
    """(stream, starts, payloads, max_symbols): self-describing preambled frames of mixed lengths,
    coding rates and CRC flags after the given gaps, no noise, no offset; made once per shape."""
    key = (sf, osr, gaps)
    if key not in _streams:
        rng = np.random.default_rng(77 + sf)
        step = (1 << sf) * osr
        frames, payloads, longest = [], [], 8
        for j in range(len(gaps)):
            pl = bytes(rng.integers(0, 256, int(rng.integers(1, 7)), dtype=np.uint8).tolist())
            syms = fc.encode_frame(pl, sf, (1, 4, 2)[j % 3], (1, 0, 1)[j % 3])
            longest = max(longest, len(syms))
            payloads.append(pl)
            frames.append((pc.frame_host(O, syms, sf, osr, 8), 8 * step))
        x, starts = pc.plant(O, frames, sf, osr, gaps, 0.0, 0.0, rng)
        _streams[key] = (x, starts, payloads, longest)
    return _streams[key]


def test_sweep_hook(amd):
    """awgn.sweep_receive_preamble(propagate=...): None changes no record; a whole-sample delay moves
    every frame and every frame still counts, by the channel's rule, with its payload; the record
    carries the channel."""
    from lora_phy_amd import awgn

    kw = dict(frames=8, max_bytes=6, seed=5)
    a = awgn.sweep_receive_preamble(7, [12.0], **kw)
    b = awgn.sweep_receive_preamble(7, [12.0], propagate=None, **kw)
    assert a == b and a[0]["returned_ok"] == 8 and "propagate" not in a[0]
    r, = awgn.sweep_receive_preamble(7, [12.0], propagate=dict(delay=3.0), **kw)
    assert r["propagate"] == {"delay": 3.0}
    assert r["planted"] == 8 and r["returned_ok"] == 8 and r["found_at_planted"] == 8 and r["cfo_right"] == 8, r
    assert r["false_frames"] == 0, r
    # seven samples are seven chips at osr 1: the frames are found where the channel put them, so a
    # start seven later counts and the planted sample itself would not
    r, = awgn.sweep_receive_preamble(7, [12.0], propagate=dict(delay=[7.0, 7.0], gain=[0.5, 0.5]), **kw)
    assert r["propagate"] == {"delay": [7.0, 7.0], "gain": [0.5, 0.5]}
    assert r["returned_ok"] == 8 and r["found_at_planted"] == 8 and r["false_frames"] == 0, r
    # a carrier offset of whole bins is what cfo_right then asks for, given as cycles or as a word
    step = 1 << 7
    for cfo in (3.0 / step, amd.stream.cfo_word64(3.0 / step)):
        r, = awgn.sweep_receive_preamble(7, [12.0], propagate=dict(cfo=cfo), **kw)
        assert r["returned_ok"] == 8 and r["cfo_right"] == 8, r
    # what the scoring cannot read is refused, not scored wrongly
    with pytest.raises(TypeError):
        awgn.sweep_receive_preamble(7, [12.0], propagate=dict(delay=torch.zeros(1, device="cuda")), **kw)
    with pytest.raises(ValueError):
        awgn.sweep_receive_preamble(7, [12.0], propagate=dict(cfo=[0.0, 0.01]), **kw)
    with pytest.raises(ValueError):
        awgn.sweep_receive_preamble(7, [12.0], propagate=dict(sfo_ppm=[1.0, 2.0, 3.0]), **kw)


@pytest.mark.parametrize("case", sorted(CASES))
def test_chain_on_propagated_rows_equals_the_host_chain(O, amd, case):
    sf, osr, gaps, channel, moved, all_back = CASES[case]
    x, planted, payloads, longest = clean_stream(O, sf, osr, gaps)
    step = (1 << sf) * osr
    hop, m = step // 4, 6
    y = amd.stream.propagate(torch.from_numpy(x).cuda(), length=len(x) + 8, **channel)
    plan = amd.DemodPlan(sf, osr, dechirp=True)
    got = amd.stream.receive_preamble_frames_device(plan, y, longest, m, hop, thresh_up_db=0.0, thresh_dn_db=0.0)
    torch.cuda.synchronize()
    y_host = y.cpu().numpy()
    # the rows are the definition's
    d = np.atleast_1d(np.asarray(channel["delay"], np.float64))
    g = np.atleast_1d(np.asarray(channel.get("gain", 1.0), np.complex64))
    ref = pp.propagate_host(x, len(x) + 8, delay=[[pp.delay_word(v) for v in d]], gain=[g.tolist()])
    assert np.array_equal(y_host.view(np.uint32), ref.view(np.uint32))

    want = pc.receive_host(O, y_host, sf, osr, longest, hop, m, 0.0, 0.0)
    if all_back:
        assert want["starts"].tolist() == (planted + moved).tolist()
        assert want["cfo_bins"].tolist() == [0] * len(planted)
        for f, pl in zip(want["frames"], payloads):
            assert f["status"] == fc.OK and bytes(f["payload"][:f["nbytes"]].tolist()) == pl
    K = len(want["starts"])
    cap = got.found.starts.shape[1]
    assert int(got.candidates[0]) == len(want["candidates"])
    assert int(got.found.count[0]) == K and int(got.found.end[0]) == want["end"]
    assert np.array_equal(got.found.starts[0].cpu().numpy(), fc.to_slots(want["starts"], cap, -1, np.int64))
    assert np.array_equal(got.cfo_bins[0].cpu().numpy(), fc.to_slots(want["cfo_bins"], cap, 0, np.int32))
    assert np.array_equal(got.nsym[0].cpu().numpy(), fc.to_slots(want["nsym"], cap, 0, np.int32))
    for j, f in enumerate(want["frames"]):
        assert int(got.frames.status[j]) == f["status"] and int(got.frames.nbytes[j]) == f["nbytes"], j
        assert np.array_equal(got.frames.payload[j].cpu().numpy()[:len(f["payload"])],
                              f["payload"][:got.frames.payload.shape[1]]), j
