"""GPU: the sliding detector scan (k_detect_scan behind lora_detect_scan_batch and
DemodPlan.scan) against the host model (tests/scan_checker.py: the existing detector checker
on every window) and against the existing kernel on materialised windows.  Every float is
compared by its bit pattern."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import detect_checker as dc
from tests import scan_checker as sc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FLOATS = ("power", "power_avg", "f_index")
DTYPES = (("power", torch.float32), ("power_avg", torch.float32), ("f_index", torch.float32), ("index", torch.uint16))


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


def host(met):
    torch.cuda.synchronize()
    return {k: getattr(met, k).cpu().numpy() for k in sc.FIELDS}


def assert_bits(got, want, what=""):
    assert got["index"].shape == want["index"].shape, (what, got["index"].shape, want["index"].shape)
    assert np.array_equal(got["index"], want["index"]), (what, "index", np.argwhere(got["index"] != want["index"])[:4])
    for k in FLOATS:
        g, w = dc.bits(got[k]), dc.bits(want[k])
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (what, k, len(bad), bad[:4].tolist(),
                               [(got[k][tuple(b)], want[k][tuple(b)]) for b in bad[:4]])


def group(sf):
    """windows per workgroup (csrc/lora_internal.h metrics_group)"""
    return 4096 >> sf if sf >= 6 else 64


def noisy_stream(O, sf, osr, L, seed, bw=125000, rows=1):
    """[rows, L]: per row a modulated frame of random symbols with noise on it, cut or padded to
    L at a random offset, the rest exact silence (windows of zeros, and windows half in it)."""
    rng = np.random.default_rng(seed)
    step = (1 << sf) * osr
    out = np.zeros((rows, L), np.complex64)
    for r in range(rows):
        nsym = max(1, (L * 2 // 3) // step - 2)
        f = O.lora_modulate(rng.integers(0, 1 << sf, nsym).astype(np.uint16), sf, osr, bw, 1.0, 0x12)
        f = (f + 0.2 * (rng.standard_normal(len(f)) + 1j * rng.standard_normal(len(f)))).astype(np.complex64)
        at = int(rng.integers(0, max(L // 5, 1)))
        n = min(len(f), L - at)
        out[r, at:at + n] = f[:n]
    return out


def length_for(sf, osr, hop, W, extra=0):
    return (1 << sf) * osr + (W - 1) * hop + extra


def hops(sf, osr=1):
    step = (1 << sf) * osr
    return list(dict.fromkeys([1, 3, max(step // 4, 1), step, step + 5]))  # (SF2: step / 4 is 1)


GRID = [(sf, h) for sf in (2, 4, 6, 7, 9) for h in hops(sf)]


@pytest.mark.parametrize("sf,hop", GRID)
def test_against_the_host_model(O, amd, sf, hop):
    """Two workgroups and a part of a third (so the window count is no multiple of G), the
    row a little longer than its last window."""
    W = min(2 * group(sf) + 3, 400)
    L = length_for(sf, 1, hop, W, extra=min(hop - 1, 2))
    x = noisy_stream(O, sf, 1, L, 100 * sf + hop)
    plan = amd.DemodPlan(sf, dechirp=True, mode="raw")
    assert plan.scan_windows(L, hop) == W
    got = host(plan.scan(torch.from_numpy(x[0]).cuda(), hop))
    assert_bits(got, sc.scan_host(O, x, sf, 1, hop, dechirp=True), f"SF{sf} hop {hop}")


@pytest.mark.parametrize("hop,W", [(2048, 5), (1000, 8)])
def test_sf12_against_the_host_model(O, amd, hop, W):
    L = length_for(12, 1, hop, W, extra=7)
    x = noisy_stream(O, 12, 1, L, hop)
    plan = amd.DemodPlan(12, dechirp=True)  # a legacy plan: the mode is ignored
    got = host(plan.scan(torch.from_numpy(x[0]).cuda(), hop))
    assert_bits(got, sc.scan_host(O, x, 12, 1, hop, dechirp=True))


# hop a multiple of osr (the staged grid of pitch osr), not one (pitch 1), one whose segment
# does not fit the staging buffer, and one beyond the window
@pytest.mark.parametrize("osr,hop", [(2, 64), (2, 3), (2, 96), (2, 65), (2, 256), (2, 261),
                                     (4, 128), (4, 5), (4, 6), (4, 132), (4, 517)])
def test_oversampled_against_the_host_model(O, amd, osr, hop):
    W = 2 * group(7) + 5
    L = length_for(7, osr, hop, W, extra=1)
    x = noisy_stream(O, 7, osr, L, 10 * osr + hop)
    plan = amd.DemodPlan(7, osr, dechirp=True, mode="raw")
    got = host(plan.scan(torch.from_numpy(x[0]).cuda(), hop))
    assert_bits(got, sc.scan_host(O, x, 7, osr, hop, dechirp=True), f"osr {osr} hop {hop}")


@pytest.mark.parametrize("hann", [False, True])
@pytest.mark.parametrize("dechirp", [False, True])
@pytest.mark.parametrize("hop", [3, 32])
def test_window_and_dechirp_options(O, amd, hann, dechirp, hop):
    W = group(7) + 9
    x = noisy_stream(O, 7, 1, length_for(7, 1, hop, W), 7 + hop)
    plan = amd.DemodPlan(7, window="hann" if hann else "none", dechirp=dechirp, mode="api")  # mode ignored
    got = host(plan.scan(torch.from_numpy(x[0]).cuda(), hop))
    assert_bits(got, sc.scan_host(O, x, 7, 1, hop, hann=hann, dechirp=dechirp))


def test_bw250(O, amd):
    hop, W = 16, group(8) + 3
    x = noisy_stream(O, 8, 1, length_for(8, 1, hop, W), 250, bw=250000)
    plan = amd.DemodPlan(8, bw=250000, dechirp=True, mode="raw")
    got = host(plan.scan(torch.from_numpy(x[0]).cuda(), hop))
    assert_bits(got, sc.scan_host(O, x, 8, 1, hop, dechirp=True, bw=250000))


@pytest.mark.parametrize("hop", [32, 100])
def test_three_rows_of_a_wider_tensor(O, amd, hop):
    """rows = 3 with row_stride > row_len: each row's last workgroup ends at the row's end, and
    the samples behind it (the padding, then the next row) are not its windows."""
    W = group(7) + 5
    L = length_for(7, 1, hop, W, extra=hop - 1)
    x = noisy_stream(O, 7, 1, L, 3 + hop, rows=3)
    wide = torch.full((3, L + 37), 1e3 + 1e3j, dtype=torch.complex64, device="cuda")
    wide[:, :L] = torch.from_numpy(x).cuda()
    plan = amd.DemodPlan(7, dechirp=True, mode="raw")
    got = host(plan.scan(wide[:, :L], hop))
    assert got["index"].shape == (3, W)
    assert_bits(got, sc.scan_host(O, x, 7, 1, hop, dechirp=True))


@pytest.mark.parametrize("offset", [1, 2, 5])
@pytest.mark.parametrize("hop", [1, 7, 32])
def test_a_view_at_an_odd_sample_offset(O, amd, offset, hop):
    """The stream begins 8 bytes (odd offsets) or 16 bytes into a larger tensor: the 16-byte
    loads of the staging pass need their alignment guard at both ends."""
    W = group(7) + 2
    L = length_for(7, 1, hop, W)
    x = noisy_stream(O, 7, 1, L, offset * 50 + hop)
    big = torch.full((L + 11,), 1e3 - 1e3j, dtype=torch.complex64, device="cuda")
    big[offset:offset + L] = torch.from_numpy(x[0]).cuda()
    plan = amd.DemodPlan(7, dechirp=True, mode="raw")
    got = host(plan.scan(big[offset:offset + L], hop))
    assert_bits(got, sc.scan_host(O, x, 7, 1, hop, dechirp=True), f"offset {offset} hop {hop}")


def test_one_window_none_and_padded_outputs(O, amd):
    sf, hop, step = 7, 32, 128
    plan = amd.DemodPlan(sf, dechirp=True, mode="raw")
    x = noisy_stream(O, sf, 1, step + hop - 1, 1)          # W == 1
    xt = torch.from_numpy(x[0]).cuda()
    want = sc.scan_host(O, x, sf, 1, hop, dechirp=True)
    assert want["index"].shape == (1, 1)
    assert_bits(host(plan.scan(xt, hop)), want, "W == 1")
    assert_bits(host(plan.scan(xt, 10 ** 12)), want, "a hop beyond the row")

    def sentinels(rows, cols):
        return amd.DetectMetrics(*(torch.full((rows, cols), 7.5, device="cuda") for _ in range(3)),
                                 torch.full((rows, cols), 0xABCD, dtype=torch.uint16, device="cuda"))

    # W == 0: nothing is launched, the outputs stay as they were
    out = sentinels(1, 4)
    assert plan.scan(xt[:step - 1], hop, out=out) is out
    got = host(out)
    assert all((got[k] == 7.5).all() for k in FLOATS) and (got["index"] == 0xABCD).all()
    assert plan.scan(xt[:step - 1], hop).power.shape == (1, 0)
    assert plan.scan(torch.zeros((0, 500), dtype=torch.complex64, device="cuda"), hop).index.shape == (0, 12)
    # out.stride > W on two rows: the padding keeps its sentinels
    W = group(sf) + 1
    x2 = noisy_stream(O, sf, 1, length_for(sf, 1, hop, W), 2, rows=2)
    want2 = sc.scan_host(O, x2, sf, 1, hop, dechirp=True)
    out = sentinels(2, W + 3)
    plan.scan(torch.from_numpy(x2).cuda(), hop, out=out)
    got = host(out)
    assert_bits({k: v[:, :W] for k, v in got.items()}, want2, "padded")
    assert all((got[k][:, W:] == 7.5).all() for k in FLOATS) and (got["index"][:, W:] == 0xABCD).all()
    # each output alone, the others NULL
    for k, dt in DTYPES:
        one = amd.DetectMetrics(None, None, None, None)
        setattr(one, k, torch.zeros((2, W), dtype=dt, device="cuda"))
        plan.scan(torch.from_numpy(x2).cuda(), hop, out=one)
        torch.cuda.synchronize()
        g = getattr(one, k).cpu().numpy()
        assert np.array_equal(g if k == "index" else dc.bits(g), want2[k] if k == "index" else dc.bits(want2[k])), k
    with pytest.raises(ValueError):
        plan.scan(xt, 0)
    with pytest.raises(ValueError):
        plan.scan(torch.from_numpy(x2).cuda(), hop, out=amd.DetectMetrics(torch.zeros((2, W - 1), device="cuda"),
                                                                           None, None, None))


def test_capi_rules_with_a_plan(amd):
    from lora_phy_amd import _capi

    lib = _capi.lib()
    step, hop, rows = 128, 32, 2
    L = step + 3 * hop
    W = 4
    plan = amd.DemodPlan(7, dechirp=True)
    h = plan._h
    # lora_detect_scan_windows: host arithmetic
    for row_len, want in ((0, 0), (step - 1, 0), (step, 1), (step + hop - 1, 1), (step + hop, 2), (L, W)):
        assert lib.lora_detect_scan_windows(h, row_len, hop) == want == sc.scan_windows(row_len, step, hop)
    assert lib.lora_detect_scan_windows(h, 2 * step + 5, step + 5) == 2
    E = _capi.LORA_EINVAL
    assert lib.lora_detect_scan_windows(h, -1, hop) == E and lib.lora_detect_scan_windows(h, L, 0) == E
    assert lib.lora_detect_scan_windows(None, L, hop) == E

    iq = torch.zeros((rows, L), dtype=torch.complex64, device="cuda")
    buf = torch.full((rows, W), 3.0, device="cuda")

    def call(rows=rows, row_len=L, stride=L, hop=hop, ostride=W, iqp=iq, power=buf, out=True):
        m = _capi.SymbolMetrics(power.data_ptr() if power is not None else None, None, None, None, ostride)
        return lib.lora_detect_scan_batch(h, iqp.data_ptr() if iqp is not None else None, rows, row_len, stride, hop,
                                          C.byref(m) if out else None, None)

    assert call(out=False) == E and lib.lora_last_error().decode()
    assert call(iqp=None) == E
    assert call(rows=-1) == E and call(row_len=-1) == E and call(stride=-1) == E and call(ostride=-1) == E
    assert call(hop=0) == E and call(hop=-1) == E
    assert call(row_len=1 << 31, stride=1 << 31) == E
    assert call(stride=L - 1) == E
    assert call(ostride=W - 1) == E
    assert call(rows=1 << 31) == E  # a grid beyond 2^31
    torch.cuda.synchronize()
    assert (buf == 3.0).all()  # nothing ran
    # no launch: rows == 0 (iq may be NULL), W == 0 (iq may be NULL), no output given - all return W
    assert call(rows=0, iqp=None) == W
    assert call(row_len=step - 1, stride=step - 1, iqp=None) == 0
    assert call(power=None, ostride=0) == W
    torch.cuda.synchronize()
    assert (buf == 3.0).all()
    # one row with any row_stride
    assert call(rows=1, stride=0) == W
    torch.cuda.synchronize()
    assert (buf[1] == 3.0).all() and not (buf[0] == 3.0).any()


def noisy_frames_on_device(amd, sf, L, seed):
    """[L] on the device: back-to-back modulated frames of 6 random symbols plus noise, a
    silent stretch in the middle."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    frame = 8 << sf
    F = L // frame + 1
    syms = torch.randint(0, 1 << sf, (F, 6), generator=g, dtype=torch.int32)
    x = amd.modulate(syms.cuda(), sf).reshape(-1)[:L].clone()
    x += 0.3 * torch.randn(L, generator=g, dtype=torch.complex64).cuda()
    x[L // 2:L // 2 + 3 * (1 << sf) + 1] = 0
    return x


# SF7 hop 5, SF9 hop 64: staged segments; SF7 hop 96 (31 * 96 + 128 samples) and SF12: direct
@pytest.mark.parametrize("sf,L,hop,hann", [(7, 100003, 5, False), (7, 100003, 96, True), (9, 1 << 16, 64, False),
                                           (12, 1 << 18, 512, False)])
def test_equals_the_existing_kernel_on_materialised_windows(amd, sf, L, hop, hann):
    step = 1 << sf
    x = noisy_frames_on_device(amd, sf, L, sf + hop)
    plan = amd.DemodPlan(sf, window="hann" if hann else "none", dechirp=True, mode="raw")
    got = host(plan.scan(x, hop))
    want = host(plan.detect_metrics(x.unfold(0, step, hop).contiguous()))
    W = (L - step) // hop + 1
    assert got["index"].shape == (1, W)
    assert_bits(got, {k: v.reshape(1, W) for k, v in want.items()})
    assert len(np.unique(got["index"])) > 4  # (not a constant)


def test_golden_capture_excerpt(O, amd):
    x = np.fromfile(os.path.join(GOLD, "capture_sf7_excerpt.iq"), dtype=np.complex64)[:4096]
    plan = amd.DemodPlan(7, 2, dechirp=True, mode="raw")
    got = host(plan.scan(torch.from_numpy(x).cuda(), 64))
    assert got["index"].shape == (1, 61)
    assert_bits(got, sc.scan_host(O, x, 7, 2, 64, dechirp=True))


def test_graph_capture_and_replay(amd):
    hop = 32
    x = noisy_frames_on_device(amd, 7, 5000, 1)
    x2 = noisy_frames_on_device(amd, 7, 5000, 2)
    plan = amd.DemodPlan(7, dechirp=True)
    out = plan.scan(x, hop)
    eager = host(out)
    eager2 = host(plan.scan(x2, hop))
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        plan.scan(x, hop, out=out)
    torch.cuda.current_stream().wait_stream(s)
    for t in (out.power, out.power_avg, out.f_index, out.index):
        t.zero_()
    with torch.cuda.graph(g):
        plan.scan(x, hop, out=out)
    g.replay()
    assert_bits(host(out), eager)
    g.replay()
    assert_bits(host(out), eager)
    x.copy_(x2)  # new samples in the captured buffer
    g.replay()
    assert_bits(host(out), eager2)
