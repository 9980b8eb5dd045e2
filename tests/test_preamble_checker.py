"""CPU: the host model of preambled frames (tests/preamble_checker.py) against the things it must
agree with before the GPU tests lean on it - the existing modulator's frame, the plain scan's host
model, the existing host selection - and the finder's rule on the table of planted streams: every
planted (start, round(cfo)) and nothing else, with thresholds 0 and max_cfo_bins = N/4 - 1."""
import numpy as np
import pytest

from tests import detect_checker as dc
from tests import frame_checker as fc
from tests import preamble_checker as pc
from tests import scan_checker as sc


@pytest.fixture(scope="module")
def O():
    from oracle.pyoracle import Oracle

    return Oracle()


@pytest.mark.parametrize("sf,osr,P,S", [(7, 1, 8, 10), (7, 2, 4, 3), (9, 1, 6, 9)])
def test_gathered_sync_and_data_equal_the_modulators_frame(O, sf, osr, P, S):
    rng = np.random.default_rng(sf * 10 + osr)
    step = (1 << sf) * osr
    syms = rng.integers(0, 1 << sf, S).astype(np.uint16)
    f = pc.frame_host(O, syms, sf, osr, P)
    assert len(f) == (P + 2 + S) * step + pc.tail_of(step)
    x = np.concatenate([np.zeros(13, np.complex64), f, np.zeros(5, np.complex64)])
    got = pc.gather_sync_data(x, 13 + P * step, step, S * step, (2 + S) * step)
    want = O.lora_modulate(syms, sf, osr, 125000, 1.0, 0x12)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # the tables are chains from phase 0: the first preamble chirp is the plain up-chirp
    pre, sfd = pc.tables_host(O, sf, osr, P)
    up0, _ = O.gen_chirp(1 << sf, osr, step, 0.0, False, 1.0, 0.0, 1.0)
    assert len(pre) == P * step and len(sfd) == pc.tail_of(step)
    assert np.array_equal(pre[:step].view(np.uint32), up0.view(np.uint32))
    assert np.array_equal(f[:P * step].view(np.uint32), pre.view(np.uint32))
    assert np.array_equal(f[(P + 2) * step:(P + 2) * step + len(sfd)].view(np.uint32), sfd.view(np.uint32))


@pytest.mark.parametrize("sf,osr,hop", [(7, 1, 32), (7, 2, 64), (8, 1, 37)])
def test_acc_1_is_the_plain_scan(O, sf, osr, hop):
    rng = np.random.default_rng(sf + hop)
    x, _, _ = sc.planted_stream(O, sf, osr, 3, (17, 40), 0.2, 0x12, sf + hop)
    x = x[:6 * (1 << sf) * osr + 11]
    want = sc.scan_host(O, x, sf, osr, hop, False, True)
    got = pc.scan_acc_host(O, x, sf, osr, hop, 1)
    assert np.array_equal(got["index"], want["index"])
    for k in ("power", "power_avg"):
        assert np.array_equal(dc.bits(got[k]), dc.bits(want[k])), k
    # and the conjugated scan is the scan of the conjugated stream
    gc = pc.scan_acc_host(O, x, sf, osr, hop, 1, conj=True)
    wc = sc.scan_host(O, np.conj(x), sf, osr, hop, False, True)
    assert np.array_equal(gc["index"], wc["index"]) and np.array_equal(dc.bits(gc["power"]), dc.bits(wc["power"]))
    del rng


def test_window_counts():
    assert pc.scan_acc_windows(128 * 3, 128, 32, 1) == 9
    assert pc.scan_acc_windows(128 * 3, 128, 32, 2) == 5
    assert pc.scan_acc_windows(128 * 3, 128, 32, 3) == 1
    assert pc.scan_acc_windows(128 * 3, 128, 32, 4) == 0
    assert pc.scan_acc_windows(100, 128, 32, 2) == 0


@pytest.mark.parametrize("ci", range(len(pc.TABLE)))
def test_finder_model_returns_every_planted_pair_and_nothing_else(O, ci):
    sf, osr, k, P, m, S, gaps, sigma, cfo = pc.TABLE[ci]
    step = (1 << sf) * osr
    hop = step // k
    x, want, _ = pc.planted_stream(O, ci)
    up = pc.scan_acc_host(O, x, sf, osr, hop, m)
    dn = pc.scan_acc_host(O, x, sf, osr, hop, 2, conj=True)
    got = pc.find_preamble_host(up, dn, hop, sf, osr, m, 0.0, 0.0, None, len(x))
    assert got.tolist() == want.tolist(), (got.tolist(), want.tolist())


def test_alias_a_quarter_symbol_off_is_rejected_by_max_cfo_bins():
    """Metrics made by hand: up and down peaks that solve to (d, c) and, N/2 away in both, to the
    alias - the rule keeps the pair within max_cfo_bins and drops the other."""
    sf, osr, k, m = 7, 1, 4, 6
    N, hop = 128, 32
    lag = (2 + m) * k
    Wd = lag + 3 * k
    Wu = Wd
    w = lag + k

    def metrics(W, idx_at, idx):
        p = np.full(W, -10.0, np.float32)
        p[idx_at] = 5.0
        i = np.zeros(W, np.uint16)
        i[idx_at] = idx
        return {"index": i, "power": p, "power_avg": np.full(W, -20.0, np.float32)}

    d, c = 10, 7
    row_len = (Wd - 1) * hop + 2 * N + 100000
    up, dn = metrics(Wu, w - lag, (d + c) % N), metrics(Wd, w, (d - c) % N)
    got = pc.find_preamble_host(up, dn, hop, sf, osr, m, 0.0, 0.0, None, row_len)
    assert got.tolist() == [[w * hop - d * osr - 2 * N, c]]
    # a window a quarter symbol off under the same offset: d' = d + N/4 makes s = 2 d' leave
    # [-N/2, N/2) and the rule solves to (d' - N/2, c + N/2) mod N, whose |c| is beyond N/4 - 1
    d2 = d + N // 4 + N // 8
    up, dn = metrics(Wu, w - lag, (d2 + c) % N), metrics(Wd, w, (d2 - c) % N)
    assert len(pc.find_preamble_host(up, dn, hop, sf, osr, m, 0.0, 0.0, None, row_len)) == 0
    # (without the bound the model would list the alias: that is what the bound is for)
    wide = pc.find_preamble_host(up, dn, hop, sf, osr, m, 0.0, 0.0, N // 2, row_len)
    assert wide.tolist() == [[w * hop - (d2 - N // 2) * osr - 2 * N, c - N // 2]]


def test_selection_with_no_tail_is_the_existing_selection():
    rng = np.random.default_rng(5)
    step, row_len = 128, 40000
    starts = np.sort(rng.integers(-1, row_len, 200)).astype(np.int64)
    status = rng.integers(0, 3, 200).astype(np.int32)
    nsym = rng.integers(-1, 40, 200).astype(np.int32)
    words = rng.integers(-50, 50, 200).astype(np.int32)
    for first in (0, 3000):
        a = fc.select_frames_host(starts, status, nsym, step, row_len, 30, first)
        b = pc.select_preamble_host(starts, words, status, nsym, step, 0, row_len, 30, first)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[2]) and a[2] == b[3]
        assert len(b[0]) > 3
    # with a tail, frames keep that much more distance and each word is its slot's own
    t = pc.select_preamble_host(starts, words, status, nsym, step, 288, row_len, 30, 0)
    assert len(t[0]) > 3 and np.all(np.diff(t[0]) >= (2 + t[2][:-1]) * step + 288)
    assert t[3] == t[0][-1] + (2 + t[2][-1]) * step + 288
    for s, wd in zip(t[0], t[1]):
        assert wd in words[starts == s]


def test_derotation_word():
    assert pc.derotation_word(0, 128) == 0
    assert pc.derotation_word(1, 128) == -(1 << 25)
    assert pc.derotation_word(-3, 256) == 3 << 24
    assert pc.derotation_word(64, 128) == -(1 << 31)
    assert pc.derotation_word(5, 384) == -((5 << 32) // 384) - 1  # floor, not truncation


@pytest.mark.parametrize("ci", [1, 5])
def test_host_chain_returns_every_planted_frame_with_its_payload(O, ci):
    sf, osr, k, P, m, S, gaps, sigma, cfo = pc.TABLE[ci]
    hop = (1 << sf) * osr // k
    x, want, payloads, longest = pc.packet_stream(O, ci)
    got = pc.receive_host(O, x, sf, osr, longest, hop, m)
    assert got["starts"].tolist() == want[:, 0].tolist()
    assert got["cfo_bins"].tolist() == want[:, 1].tolist()
    for f, pl in zip(got["frames"], payloads):
        assert f["status"] == fc.OK and f["nbytes"] == len(pl)
        assert bytes(f["payload"][:len(pl)].tolist()) == pl
