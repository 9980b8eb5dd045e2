"""GPU: the preambled receive chain (stream.receive_preamble_frames_device) against its host model
(tests/preamble_checker.receive_host: the oracle's FFT and demodulator, impair_checker's rotation,
frame_checker's gate and decode) as integers - starts, cfo_bins, nsym, status, payload, symbols -
hard and soft, after the host chain has been shown to return every planted frame with its payload;
and the loop-back LoRaMod.work_frame(preamble=8) -> impair(cfo=...) -> the chain."""
import numpy as np
import pytest

from tests import frame_checker as fc
from tests import preamble_checker as pc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


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


@pytest.mark.parametrize("thresh", [0.0, None])  # explicit, and the chain's measured default
@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("ci", [1, 5, 7])  # SF7 at 5 bins, SF7 osr 2 at 4 bins, SF9 at -20.4 bins
def test_chain_equals_the_host_chain(O, amd, ci, soft, thresh):
    sf, osr, k, P, m, S, gaps, sigma, cfo = pc.TABLE[ci]
    step = (1 << sf) * osr
    hop = step // k
    x, planted, payloads, longest = pc.packet_stream(O, ci)
    th = amd.stream.preamble_threshold_db(sf) if thresh is None else thresh
    assert thresh is not None or th == {7: -10.0, 9: -16.0}[sf]
    want = pc.receive_host(O, x, sf, osr, longest, hop, m, th, th, soft=soft)
    # the host chain finds every planted frame, its offset and its payload
    assert want["starts"].tolist() == planted[:, 0].tolist()
    assert want["cfo_bins"].tolist() == planted[:, 1].tolist()
    for f, pl in zip(want["frames"], payloads):
        assert f["status"] == fc.OK and bytes(f["payload"][:f["nbytes"]].tolist()) == pl

    plan = amd.DemodPlan(sf, osr, dechirp=True)
    got = amd.stream.receive_preamble_frames_device(plan, torch.from_numpy(x).cuda(), longest, m, hop,
                                                    thresh_up_db=thresh, thresh_dn_db=thresh, soft=soft)
    torch.cuda.synchronize()
    K = len(want["starts"])
    cap = got.found.starts.shape[1]
    assert cap == len(x) // (10 * step + pc.tail_of(step)) and got.cfo_bins.shape == (1, cap)
    assert int(got.candidates[0]) == len(want["candidates"])
    assert int(got.found.count[0]) == K and int(got.found.end[0]) == want["end"]
    assert np.array_equal(got.found.starts[0].cpu().numpy(), fc.to_slots(want["starts"], cap, -1, np.int64))
    assert np.array_equal(got.cfo_bins[0].cpu().numpy(), fc.to_slots(want["cfo_bins"], cap, 0, np.int32))
    assert np.array_equal(got.nsym[0].cpu().numpy(), fc.to_slots(want["nsym"], cap, 0, np.int32))
    syms = got.result.symbols.cpu().numpy()
    assert (got.llr is not None) == soft
    for j, f in enumerate(want["frames"]):
        assert int(got.frames.status[j]) == f["status"] and int(got.frames.nbytes[j]) == f["nbytes"], j
        assert int(got.frames.rdd[j]) == f["rdd"] and int(got.frames.has_crc[j]) == f["crc"], j
        assert np.array_equal(got.frames.payload[j].cpu().numpy()[:len(f["payload"])],
                              f["payload"][:got.frames.payload.shape[1]]), j
        assert np.array_equal(syms[j, :len(f["symbols"])], f["symbols"]), j
        assert int(got.result.sync[j]) == f["sync"], j
        assert np.float32(got.result.cfo[j].item()).view(np.uint32) == np.float32(f["cfo"]).view(np.uint32), j


def test_rows_shorter_than_a_frame_and_two_rows(O, amd):
    sf, osr, k, P, m = 7, 1, 4, 8, 6
    plan = amd.DemodPlan(sf, dechirp=True)
    got = amd.stream.receive_preamble_frames_device(plan, torch.zeros(300, dtype=torch.complex64, device="cuda"), 20)
    torch.cuda.synchronize()
    assert got.found.starts.shape == (1, 0) and int(got.found.count[0]) == 0 and int(got.candidates[0]) == 0
    # two rows of a wider tensor: row 0 the planted stream, row 1 silence with the same frames later
    x, planted, payloads, longest = pc.packet_stream(O, 1)
    L = len(x) + 200
    wide = torch.zeros((2, L + 9), dtype=torch.complex64, device="cuda")
    wide[0, :len(x)] = torch.from_numpy(x).cuda()
    wide[1, 200:200 + len(x)] = torch.from_numpy(x).cuda()
    got = amd.stream.receive_preamble_frames_device(plan, wide[:, :L], longest, m)
    torch.cuda.synchronize()
    K = len(planted)
    assert got.found.count.tolist() == [K, K]
    assert got.found.starts[0, :K].tolist() == planted[:, 0].tolist()
    assert got.found.starts[1, :K].tolist() == (planted[:, 0] + 200).tolist()
    assert got.cfo_bins[:, :K].tolist() == [planted[:, 1].tolist()] * 2
    cap = got.found.starts.shape[1]
    for r in range(2):
        for j, pl in enumerate(payloads):
            s = r * cap + j
            assert int(got.frames.status[s]) == fc.OK and int(got.frames.nbytes[s]) == len(pl)
            assert bytes(got.frames.payload[s, :len(pl)].cpu().tolist()) == pl


@pytest.mark.parametrize("sf,bins", [(7, 9), (8, -17)])
def test_loop_back_through_the_modulator_and_the_channel(amd, sf, bins):
    """LoRaMod.work_frame(preamble=8) -> a stream with gaps -> impair(cfo=bins / step, noise) -> the
    chain: every payload back, the offset reported."""
    step = 1 << sf
    g = torch.Generator(device="cpu").manual_seed(sf)
    F, max_bytes = 5, 9
    payload = torch.randint(0, 256, (F, max_bytes), generator=g, dtype=torch.int32).to(torch.uint8)
    nbytes = torch.tensor([0, 9, 3, 7, 1], dtype=torch.int32)
    mod = amd.LoRaMod(sf, cr=2)
    plain = mod.work_frame(payload, nbytes)
    frames = mod.work_frame(payload, nbytes, preamble=8)
    tail = 9 * step // 4
    assert frames.shape == (F, plain.shape[1] + 8 * step + tail)
    # [sync | data] of a preambled frame is the plain frame, bit for bit
    back = torch.cat([frames[:, 8 * step:10 * step], frames[:, 10 * step + tail:]], dim=1)
    assert torch.equal(torch.view_as_real(back), torch.view_as_real(plain))
    gap = torch.zeros((F, 333), dtype=torch.complex64, device="cuda")
    x = torch.cat([gap, frames], dim=1).reshape(-1)
    x = torch.cat([x, torch.zeros(step, dtype=torch.complex64, device="cuda")])
    y = amd.impair(x, cfo=bins / step, sigma=0.05, seed=sf)
    max_symbols = plain.shape[1] // step - 2
    got = amd.LoRaDemod(sf).work_preamble_device(y, max_symbols)
    torch.cuda.synchronize()
    assert int(got.found.count[0]) == F
    row = frames.shape[1] + 333
    assert got.found.starts[0, :F].tolist() == [f * row + 333 + 8 * step for f in range(F)]
    assert got.cfo_bins[0, :F].tolist() == [bins] * F
    for f in range(F):
        n = int(nbytes[f])
        assert int(got.frames.status[f]) == fc.OK and int(got.frames.nbytes[f]) == n
        assert got.frames.payload[f, :n].cpu().tolist() == payload[f, :n].tolist()
