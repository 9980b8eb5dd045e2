"""GPU: stream receive (lora_phy_amd.stream: scan, find, extract, demodulate) on streams with
frames planted at known starts, against the host model (tests/scan_checker.py) and the oracle's
demodulator on the frames cut at the found starts."""
import numpy as np
import pytest

from tests import detect_checker as dc
from tests import scan_checker as sc

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


def device_stream(amd, ci):
    """The table row's stream built on the device: frames from `modulate` written into zeros,
    the host-drawn noise added over the whole stream."""
    sf, osr, k, S, gaps, sigma, sync = sc.TABLE[ci]
    rng = np.random.default_rng(sc.table_seed(ci) + 500)
    starts, L = sc.planted_layout(sf, osr, S, gaps)
    syms = rng.integers(0, 1 << sf, (len(gaps), S)).astype(np.uint16)
    frames = amd.modulate(torch.from_numpy(syms.astype(np.int32)).cuda(), sf, osr, 125000, 1.0, sync)
    x = torch.zeros(L, dtype=torch.complex64, device="cuda")
    for s, f in zip(starts.tolist(), frames):
        x[s:s + f.shape[0]] = f
    if sigma:
        n = (sigma * (rng.standard_normal(L) + 1j * rng.standard_normal(L))).astype(np.complex64)
        x += torch.from_numpy(n).cuda()
    return x, starts, syms


@pytest.mark.parametrize("ci", [0, 1, 8])
def test_receive_returns_the_planted_frames(amd, ci):
    sf, osr, k, S, gaps, sigma, sync = sc.TABLE[ci]
    assert osr == 1 and sync == 0x12
    x, starts, syms = device_stream(amd, ci)
    plan = amd.DemodPlan(sf, dechirp=True)
    got_starts, res = amd.stream.receive(plan, x, S)  # hop = step // 4
    torch.cuda.synchronize()
    assert got_starts.dtype == torch.int64 and got_starts.is_cuda
    assert got_starts.cpu().tolist() == starts.tolist()
    assert np.array_equal(res.symbols.cpu().numpy() % (1 << sf), syms)
    assert (res.sync.cpu().numpy() == 0x12).all()


@pytest.mark.parametrize("ci", range(len(sc.TABLE)))
def test_receive_equals_the_host_model_and_the_oracle(O, amd, ci):
    sf, osr, k, S, gaps, sigma, sync = sc.TABLE[ci]
    step = (1 << sf) * osr
    hop, frame_len = step // k, (S + 2) * step
    x, planted, _ = sc.planted_stream(O, sf, osr, S, gaps, sigma, sync, sc.table_seed(ci))
    plan = amd.DemodPlan(sf, osr, dechirp=True)
    starts, res = amd.stream.receive(plan, torch.from_numpy(x).cuda(), S, hop=hop, sync=sync)
    torch.cuda.synchronize()
    want = sc.find_frames_host(sc.scan_host(O, x, sf, osr, hop, dechirp=True), hop, sf, osr, S, sync, row_len=len(x))
    assert want.tolist() == planted.tolist()
    assert starts.cpu().tolist() == want.tolist()
    cut = np.stack([x[s:s + frame_len] for s in want])
    o_syms, o_sync, o_cfo, o_toff, cnt = O.demod_frames(cut, sf, osr, False, True)
    assert (np.asarray(cnt) == S).all()
    assert np.array_equal(res.symbols.cpu().numpy(), np.asarray(o_syms)[:, :S])
    assert np.array_equal(res.sync.cpu().numpy(), np.asarray(o_sync).astype(np.uint8))
    assert np.array_equal(dc.bits(res.cfo.cpu().numpy()), dc.bits(o_cfo))
    assert np.array_equal(dc.bits(res.time_offset.cpu().numpy()), dc.bits(o_toff))
    # the same frames through extract_frames
    frames = amd.stream.extract_frames(torch.from_numpy(x).cuda(), starts, frame_len)
    assert np.array_equal(frames.cpu().numpy(), cut)


def test_nothing_found_makes_no_demod_call(amd):
    plan = amd.DemodPlan(7, dechirp=True)
    x = torch.zeros(4000, dtype=torch.complex64, device="cuda")
    starts, res = amd.stream.receive(plan, x, 6)
    assert starts.shape == (0,) and starts.dtype == torch.int64
    assert res.symbols.shape == (0, 6) and res.symbols.dtype == torch.uint16
    assert res.sync.shape == res.cfo.shape == res.time_offset.shape == res.max_amp.shape == (0,)
    assert plan.last_kernels() == set()  # run() never ran on this plan
    s2, r2 = amd.stream.receive(plan, x[:100], 6)  # shorter than one window
    assert s2.shape == (0,) and r2.symbols.shape == (0, 6)
    with pytest.raises(ValueError):
        amd.stream.receive(amd.DemodPlan(7), x, 6)  # a plan that does not dechirp
    with pytest.raises(ValueError):
        amd.stream.receive(plan, x, 6, hop=48)
    with pytest.raises(ValueError):
        amd.stream.receive(amd.DemodPlan(7, bw=250000, dechirp=True), x, 6)


def test_work_stream_honours_mtu_and_sets_last(amd):
    sf, osr, k, S, gaps, sigma, sync = sc.TABLE[1]
    x, planted, syms = device_stream(amd, 1)
    demod = amd.LoRaDemod(sf, mtu=4)
    starts, got = demod.work_stream(x, S)
    torch.cuda.synchronize()
    assert starts.cpu().tolist() == planted.tolist()
    assert got.shape == (len(planted), 4) and np.array_equal(got.cpu().numpy(), syms[:, :4])
    assert demod.last is not None and np.array_equal(demod.last.symbols.cpu().numpy(), syms)
    assert demod.sync_ok().all()
    assert demod.thresh == amd.LoRaDemod.THRESH_DEFAULT
    with pytest.raises(ValueError):
        amd.LoRaDemod(sf, thresh=-20.0)  # the Pothos parameter stays as it was


def test_chunked_file_finds_a_straddling_frame_once(amd, tmp_path):
    """iter_stream and the `first` recipe of its docstring: chunks of 1500 samples cut the second
    frame (1066 .. 2090) and the fourth in two; every frame is found exactly once."""
    sf, osr, k, S, gaps, sigma, sync = sc.TABLE[1]
    x, planted, syms = device_stream(amd, 1)
    path = str(tmp_path / "stream.iq")
    assert amd.iq_io.write_iq(path, x) == x.shape[0]
    step, hop = 1 << sf, (1 << sf) // 4
    frame_len = (S + 2) * step
    chunk = 1500
    assert any(s < b < s + frame_len for s in planted.tolist() for b in range(chunk, x.shape[0], chunk))
    plan = amd.DemodPlan(sf, dechirp=True)
    found, symbols, end = [], [], 0
    for off, part in amd.iq_io.iter_stream(path, chunk, frame_len + step, device="cuda"):
        last = part.shape[0] <= chunk
        starts = amd.stream.find_frames(plan.scan(part, hop), hop, sf, osr, S, first=max(0, end - off),
                                        row_len=part.shape[0])
        if not last:
            starts = starts[starts < chunk]
        if starts.numel():
            found += (starts + off).cpu().tolist()
            end = found[-1] + frame_len
            symbols.append(plan.run(amd.stream.extract_frames(part, starts, frame_len)).symbols.cpu().numpy())
    assert found == planted.tolist()
    assert np.array_equal(np.concatenate(symbols), syms)
