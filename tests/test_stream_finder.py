"""CPU: the frame finder (lora_phy_amd.stream.find_frames) on the host model of the scan.

Streams are oracle-modulated frames (random symbols) written into zeros at planted starts,
with noise over the whole stream where the case has any (tests/scan_checker.py).  The scan is
``scan_host`` - the existing detector checker on every window - and both the product's
``find_frames`` (on CPU tensors) and the numpy restatement of its rule must return the planted
starts exactly."""
import functools

import numpy as np
import pytest

from tests import scan_checker as sc

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def O():
    from oracle.pyoracle import Oracle

    return Oracle()


@pytest.fixture(scope="module")
def stream():
    from lora_phy_amd import stream

    return stream


def as_metrics(m):
    from lora_phy_amd import DetectMetrics

    return DetectMetrics(*(torch.from_numpy(np.ascontiguousarray(m[k][0])) for k in ("power", "power_avg", "f_index",
                                                                                    "index")))


@functools.lru_cache(maxsize=None)
def _case(ci):
    from oracle.pyoracle import Oracle

    sf, osr, k, S, gaps, sigma, sync = sc.TABLE[ci]
    x, starts, syms = sc.planted_stream(Oracle(), sf, osr, S, gaps, sigma, sync, sc.table_seed(ci))
    hop = (1 << sf) * osr // k
    return x, starts, hop, sc.scan_host(Oracle(), x, sf, osr, hop, dechirp=True)


@pytest.mark.parametrize("ci", range(len(sc.TABLE)))
def test_planted_starts_are_recovered(stream, ci):
    sf, osr, k, S, gaps, sigma, sync = sc.TABLE[ci]
    x, starts, hop, m = _case(ci)
    assert m["index"].shape == (1, sc.scan_windows(len(x), (1 << sf) * osr, hop))
    host = sc.find_frames_host(m, hop, sf, osr, S, sync, row_len=len(x))
    assert host.tolist() == starts.tolist()
    got = stream.find_frames(as_metrics(m), hop, sf, osr, S, sync=sync, row_len=len(x))
    assert got.dtype == torch.int64 and got.device.type == "cpu"
    assert got.tolist() == starts.tolist()
    # [1, W] tensors and the default row_len (the span the windows cover) give the same
    from lora_phy_amd import DetectMetrics

    two_d = DetectMetrics(*(torch.from_numpy(np.ascontiguousarray(m[f])) for f in ("power", "power_avg", "f_index",
                                                                                   "index")))
    span = (m["index"].shape[1] - 1) * hop + (1 << sf) * osr
    want = sc.find_frames_host(m, hop, sf, osr, S, sync, row_len=span)
    assert stream.find_frames(two_d, hop, sf, osr, S, sync=sync).tolist() == want.tolist()


@pytest.mark.parametrize("ci", [0, 1])
def test_first_resumes_after_the_second_frame(stream, ci):
    sf, osr, k, S, gaps, sigma, sync = sc.TABLE[ci]
    x, starts, hop, m = _case(ci)
    frame_len = (S + 2) * (1 << sf) * osr
    first = int(starts[1]) + frame_len
    for f in (first, first - 1, first + 1, int(starts[2])):
        want = [s for s in starts.tolist() if s >= f]
        assert sc.find_frames_host(m, hop, sf, osr, S, sync, first=f, row_len=len(x)).tolist() == want, f
        assert stream.find_frames(as_metrics(m), hop, sf, osr, S, first=f, row_len=len(x)).tolist() == want, f
    # one sample past the third start: that frame is gone, the fourth stays
    f = int(starts[2]) + 1
    assert stream.find_frames(as_metrics(m), hop, sf, osr, S, first=f, row_len=len(x)).tolist() == [int(starts[3])]
    assert sc.find_frames_host(m, hop, sf, osr, S, sync, first=f, row_len=len(x)).tolist() == [int(starts[3])]
    # a row too short for the last frame drops it
    assert stream.find_frames(as_metrics(m), hop, sf, osr, S, row_len=len(x) - 1).tolist() == starts[:-1].tolist()


def test_threshold_gates_both_sync_windows(stream):
    sf, osr, k, S, gaps, sigma, sync = sc.TABLE[1]
    x, starts, hop, m = _case(1)
    assert stream.find_frames(as_metrics(m), hop, sf, osr, S, thresh_db=200.0, row_len=len(x)).numel() == 0
    assert sc.find_frames_host(m, hop, sf, osr, S, thresh_db=200.0, row_len=len(x)).size == 0


def test_all_zero_stream_gives_no_starts(O, stream):
    sf, hop, S = 7, 32, 2
    x = np.zeros(6 * 128, np.complex64)
    m = sc.scan_host(O, x, sf, 1, hop, dechirp=True)
    with np.errstate(invalid="ignore"):
        assert np.isnan(m["power"] - m["power_avg"]).all()
    assert sc.find_frames_host(m, hop, sf, 1, S, thresh_db=-1e30).size == 0
    got = stream.find_frames(as_metrics(m), hop, sf, 1, S, thresh_db=-1e30)
    assert got.shape == (0,) and got.dtype == torch.int64


def test_fewer_windows_than_one_symbol_apart(stream):
    from lora_phy_amd import DetectMetrics

    z = torch.zeros(3)
    m = DetectMetrics(z, z - 1, z, torch.zeros(3, dtype=torch.uint16))
    assert stream.find_frames(m, 32, 7, 1, 2).shape == (0,)
    e = torch.zeros(0)
    assert stream.find_frames(DetectMetrics(e, e, e, torch.zeros(0, dtype=torch.uint16)), 32, 7, 1, 2).shape == (0,)


@pytest.mark.parametrize("kw", [dict(sf=5), dict(sf=13), dict(hop=48), dict(hop=128), dict(hop=0), dict(hop=256),
                                dict(bw=250000), dict(osr=2, hop=96)])
def test_value_errors(stream, kw):
    from lora_phy_amd import DetectMetrics

    z = torch.zeros(40)
    m = DetectMetrics(z, z - 1, z, torch.zeros(40, dtype=torch.uint16))
    args = dict(hop=32, sf=7, osr=1, frame_symbols=2)
    stream.find_frames(m, **args)  # the base arguments are fine
    args.update(kw)
    with pytest.raises(ValueError):
        stream.find_frames(m, **args)


def test_extract_frames_gathers_and_checks_its_bounds(stream):
    x = torch.arange(50, dtype=torch.float32).to(torch.complex64)
    got = stream.extract_frames(x, torch.tensor([0, 7, 40]), 10)
    assert got.shape == (3, 10) and got.is_contiguous()
    assert got.real.tolist() == [list(range(s, s + 10)) for s in (0, 7, 40)]
    assert stream.extract_frames(x, torch.zeros(0, dtype=torch.int64), 10).shape == (0, 10)
    assert stream.extract_frames(x[3:], torch.tensor([1]), 4).real.tolist() == [[4.0, 5.0, 6.0, 7.0]]
    for bad in ([41], [-1], [0, 45]):
        with pytest.raises(ValueError):
            stream.extract_frames(x, torch.tensor(bad), 10)


def test_iter_stream_chunks_overlap(tmp_path):
    from lora_phy_amd import iq_io

    x = (np.arange(25) + 1j * np.arange(25)).astype(np.complex64)
    p = str(tmp_path / "s.iq")
    x.tofile(p)
    got = [(off, t.numpy()) for off, t in iq_io.iter_stream(p, 10, 4)]
    assert [off for off, _ in got] == [0, 10, 20]
    assert [len(t) for _, t in got] == [14, 14, 5]  # only the last holds <= chunk_samples
    for off, t in got:
        assert np.array_equal(t, x[off:off + 14])
    assert [len(t) for _, t in iq_io.iter_stream(p, 25, 4)] == [25]
    assert [len(t) for _, t in iq_io.iter_stream(p, 20, 5)] == [25, 5]
    with pytest.raises(ValueError):
        list(iq_io.iter_stream(p, 0, 4))
