"""GPU: the preamble finder (k_find_preamble behind lora_find_preamble_batch) and the selection
with a tail and a carried word (lora_select_preamble_batch) against their host models
(tests/preamble_checker.py), as integers: on the device's own accumulating scans of the table's
planted streams, and on synthetic metrics that cross the kernels' turn boundaries and exceed
the capacity.  The existing selection entry is checked unchanged on one case."""
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


def to_host(met):
    torch.cuda.synchronize()
    return {k: getattr(met, k).cpu().numpy() for k in ("index", "power", "power_avg")}


def to_device(amd, m, pad=0):
    """[R, W] metrics on the device, as views of [R, W + pad] tensors."""
    def put(a):
        a = np.atleast_2d(a)
        wide = np.zeros((a.shape[0], a.shape[1] + pad), a.dtype)
        wide[:, :a.shape[1]] = a
        return torch.from_numpy(wide).cuda()[:, :a.shape[1]]

    return amd.DetectMetrics(put(m["power"]), put(m["power_avg"]), None, put(m["index"]))


def check_rows(got, want_rows, cap):
    count, starts, cfo = (t.cpu().numpy() for t in got)
    for r, want in enumerate(want_rows):
        assert count[r] == len(want), (r, count[r], len(want))
        assert np.array_equal(starts[r], fc.to_slots(want[:, 0], cap, -1, np.int64)), r
        assert np.array_equal(cfo[r], fc.to_slots(want[:, 1], cap, 0, np.int32)), r


@pytest.mark.parametrize("ci", range(len(pc.TABLE)))
def test_table_rows_the_planted_pairs_and_the_host_model(O, amd, ci):
    sf, osr, k, P, m, S, gaps, sigma, cfo = pc.TABLE[ci]
    hop = (1 << sf) * osr // k
    x, planted, _ = pc.planted_stream(O, ci)
    xt = torch.from_numpy(x).cuda()
    plan = amd.DemodPlan(sf, osr, dechirp=True, mode="raw")
    up, dn = plan.scan_acc(xt, hop, m), plan.scan_acc(xt, hop, 2, conj=True)
    got = amd.stream.find_preamble_device(up, dn, hop, sf, osr, m, 0.0, 0.0, None, len(x))
    want = pc.find_preamble_host(to_host(up), to_host(dn), hop, sf, osr, m, 0.0, 0.0, None, len(x))
    cap = got[1].shape[1]
    assert cap == -(-len(x) // (4 * (1 << sf) * osr))
    check_rows(got, [want], cap)
    assert want.tolist() == planted.tolist()
    # a threshold no window reaches, and an offset bound below the planted offset
    none = amd.stream.find_preamble_device(up, dn, hop, sf, osr, m, 200.0, 0.0, None, len(x))
    assert int(none[0].cpu()[0]) == 0 and (none[1].cpu() == -1).all() and (none[2].cpu() == 0).all()
    if abs(round(cfo)) > 0 and abs(round(cfo)) <= (1 << sf) // 4 - 1:
        low = amd.stream.find_preamble_device(up, dn, hop, sf, osr, m, 0.0, 0.0, abs(round(cfo)) - 1, len(x))
        wlow = pc.find_preamble_host(to_host(up), to_host(dn), hop, sf, osr, m, 0.0, 0.0, abs(round(cfo)) - 1, len(x))
        check_rows(low, [wlow], cap)
        assert len(wlow) == 0


def synthetic(seed, sf, k, m, W, frac):
    """Up and down metrics that make many candidates: a share `frac` of down windows given a local
    power maximum, index pairs that solve to small offsets, runs of equal (start, c) pairs, NaN
    powers and -inf floors sprinkled in."""
    rng = np.random.default_rng(seed)
    N = 1 << sf
    lag = (2 + m) * k

    def base():
        p = rng.normal(0, 1, W).astype(np.float32)
        a = (p - rng.normal(3, 2, W).astype(np.float32)).astype(np.float32)
        return {"index": rng.integers(0, N, W).astype(np.uint16), "power": p, "power_avg": a}

    up, dn = base(), base()
    hop_chips = N // k
    for w in np.flatnonzero(rng.random(W) < frac):
        if w < lag or w + k >= W:
            continue
        dn["power"][w] = 6.0 + rng.random()
        d, c = int(rng.integers(-N // 4, N // 4)), int(rng.integers(-N // 8, N // 8))
        up["index"][w - lag], dn["index"][w] = (d + c) % N, (d - c) % N
        if rng.random() < 0.5 and w + 1 + k < W:  # the next window one hop later in the same frame
            dn["power"][w + 1] = dn["power"][w]
            up["index"][w + 1 - lag], dn["index"][w + 1] = (d + hop_chips + c) % N, (d + hop_chips - c) % N
    for m_ in (up, dn):
        m_["power"][rng.random(W) < 0.01] = np.nan
        m_["power_avg"][rng.random(W) < 0.01] = -np.inf
    return up, dn


@pytest.mark.parametrize("sf,k,m,W,cap", [(7, 4, 6, 5000, 64), (7, 4, 6, 1024 + 32 + 3, 2000), (9, 8, 2, 3000, 0),
                                          (8, 4, 8, 40, 8)])
def test_synthetic_metrics_across_turns_and_beyond_capacity(amd, sf, k, m, W, cap):
    N = 1 << sf
    hop = N // k
    rows = 3
    ups, dns = zip(*(synthetic(100 * sf + r, sf, k, m, W, 0.2) for r in range(rows)))
    row_len = (W - 1) * hop + 2 * N
    # rows of a wider tensor: a stride above the window count
    upm = {f: np.stack([u[f] for u in ups]) for f in ups[0]}
    dnm = {f: np.stack([d[f] for d in dns]) for f in dns[0]}
    up, dn = to_device(amd, upm, pad=5), to_device(amd, dnm, pad=0)
    got = amd.stream.find_preamble_device(up, dn, hop, sf, 1, m, 1.0, 2.0, N // 8, row_len, cap)
    want = [pc.find_preamble_host(ups[r], dns[r], hop, sf, 1, m, 1.0, 2.0, N // 8, row_len) for r in range(rows)]
    check_rows(got, want, cap)
    if W > 1000:  # (the lists are long, and with 64 slots longer than the capacity)
        assert min(len(w) for w in want) > 64


def test_selection_against_the_host_model_and_the_old_entry_unchanged(amd):
    rng = np.random.default_rng(11)
    R, C, step, row_len, max_symbols = 3, 700, 128, 400000, 30
    tail = pc.tail_of(step)
    starts = np.sort(rng.integers(-1, row_len, (R, C)), axis=1).astype(np.int64)
    status = rng.integers(0, 3, (R, C)).astype(np.int32)
    nsym = rng.integers(-1, 40, (R, C)).astype(np.int32)
    words = rng.integers(-60, 60, (R, C)).astype(np.int32)
    # row 0 begins with two candidates at one start with different offsets: the first states a
    # frame that is too long, the second is taken, with its own word
    starts[0, :2], status[0, :2], nsym[0, :2], words[0, :2] = 10, fc.OK, (31, 9), (-7, 12)
    first = np.array([0, 5000, 0], np.int64)
    dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    for cap in (0, 7, 400):
        found, n, w = amd.stream.select_preamble_device(dev(starts), dev(words), dev(status), dev(nsym), step, row_len,
                                                        max_symbols, dev(first), cap)
        old, on = amd.stream.select_frames_device(dev(starts), dev(status), dev(nsym), step, row_len, max_symbols,
                                                  dev(first), cap)
        torch.cuda.synchronize()
        for r in range(R):
            ws, ww, wn, wend = pc.select_preamble_host(starts[r], words[r], status[r], nsym[r], step, tail, row_len,
                                                       max_symbols, int(first[r]))
            assert int(found.count[r]) == len(ws) and int(found.end[r]) == wend
            assert np.array_equal(found.starts[r].cpu().numpy(), fc.to_slots(ws, cap, -1, np.int64))
            assert np.array_equal(n[r].cpu().numpy(), fc.to_slots(wn, cap, 0, np.int32))
            assert np.array_equal(w[r].cpu().numpy(), fc.to_slots(ww, cap, 0, np.int32))
            if cap >= 400:
                assert len(ws) > 20
            if r == 0:
                assert ws[0] == 10 and wn[0] == 9 and ww[0] == 12
            os_, on_, oend = fc.select_frames_host(starts[r], status[r], nsym[r], step, row_len, max_symbols,
                                                   int(first[r]))
            assert int(old.count[r]) == len(os_) and int(old.end[r]) == oend
            assert np.array_equal(old.starts[r].cpu().numpy(), fc.to_slots(os_, cap, -1, np.int64))
            assert np.array_equal(on[r].cpu().numpy(), fc.to_slots(on_, cap, 0, np.int32))
    # tail = 0 with words is the old pass with the word carried
    f0, n0, _ = amd.stream.select_preamble_device(dev(starts), dev(words), dev(status), dev(nsym), step, row_len,
                                                  max_symbols, dev(first), 400, tail=0)
    torch.cuda.synchronize()
    assert torch.equal(f0.starts, old.starts) and torch.equal(n0, on) and torch.equal(f0.end, old.end)
