"""GPU: the accumulating scan (k_detect_scan_acc behind lora_detect_scan_acc_batch and
DemodPlan.scan_acc).  acc = 1 against the plain scan, bit for bit, on both sides of the staging
switch; acc 2, 6, 8 against the host model (tests/preamble_checker.scan_acc_host: the oracle's FFT,
fp32 sums oldest first), floats by their bit patterns and the index as integers."""
import numpy as np
import pytest

from tests import detect_checker as dc
from tests import preamble_checker as pc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FLOATS = ("power", "power_avg")


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
    return {k: getattr(met, k).cpu().numpy() for k in ("index",) + FLOATS}


def assert_bits(got, want, what=""):
    assert got["index"].shape == want["index"].shape, (what, got["index"].shape, want["index"].shape)
    assert np.array_equal(got["index"], want["index"]), (what, "index", np.argwhere(got["index"] != want["index"])[:4])
    for k in FLOATS:
        g, w = dc.bits(got[k]), dc.bits(want[k])
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (what, k, len(bad), bad[:4].tolist(),
                               [(got[k][tuple(b)], want[k][tuple(b)]) for b in bad[:4]])


def device_stream(amd, sf, L, seed):
    """[L] on the device: back-to-back modulated frames of 6 random symbols plus noise, a silent
    stretch in the middle."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    F = L // (8 << sf) + 1
    syms = torch.randint(0, 1 << sf, (F, 6), generator=g, dtype=torch.int32)
    x = amd.modulate(syms.cuda(), sf).reshape(-1)[:L].clone()
    x += 0.3 * torch.randn(L, generator=g, dtype=torch.complex64).cuda()
    x[L // 2:L // 2 + (1 << sf) + 1] = 0
    return x


# SF7 step / 4: a staged segment; SF7 step / 2 (31 * 64 + 128 samples do not fit), SF12 (one window
# per workgroup) and SF11 step / 4: direct loads
@pytest.mark.parametrize("sf,hop,L", [(7, 32, 128 + 70 * 32 + 5), (7, 64, 128 + 70 * 64), (12, 1024, 4096 * 3 + 9),
                                      (11, 512, 2048 * 4)])
def test_acc_1_is_the_plain_scan(amd, sf, hop, L):
    x = device_stream(amd, sf, L, sf + hop)
    plan = amd.DemodPlan(sf, dechirp=True, mode="raw")
    want = host(plan.scan(x, hop))
    got = plan.scan_acc(x, hop, 1)
    assert got.f_index is None
    assert_bits(host(got), want, "acc 1")
    assert len(np.unique(want["index"])) > 2
    wantc = host(plan.scan(torch.conj(x).resolve_conj(), hop))
    assert_bits(host(plan.scan_acc(x, hop, 1, conj=True)), wantc, "acc 1 conj")


@pytest.mark.parametrize("ci", range(len(pc.TABLE)))
def test_table_rows_against_the_host_model(O, amd, ci):
    sf, osr, k, P, m, S, gaps, sigma, cfo = pc.TABLE[ci]
    hop = (1 << sf) * osr // k
    x, _, _ = pc.planted_stream(O, ci)
    xt = torch.from_numpy(x).cuda()
    plan = amd.DemodPlan(sf, osr, dechirp=True, mode="raw")
    for acc, conj in ((2, True), (6, False), (8, False)):
        got = host(plan.scan_acc(xt, hop, acc, conj=conj))
        assert got["index"].shape == (1, pc.scan_acc_windows(len(x), (1 << sf) * osr, hop, acc))
        assert_bits(got, pc.scan_acc_host(O, x, sf, osr, hop, acc, conj), f"case {ci} acc {acc}")


def noise_rows(rows, L, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((rows, L)) + 1j * rng.standard_normal((rows, L))).astype(np.complex64)


@pytest.mark.parametrize("acc", [2, 3])
def test_a_window_count_that_is_no_multiple_of_the_group(O, amd, acc):
    """Wa = 2 * G + 3 at SF7 (G = 32): two full workgroups and a part of a third, the row a little
    longer than its last window."""
    sf, hop, k = 7, 32, 4
    Wa = 67
    L = 128 + (Wa + (acc - 1) * k - 1) * hop + 7
    x = noise_rows(1, L, 40 + acc)
    plan = amd.DemodPlan(sf, dechirp=True, mode="raw")
    assert plan._lib.lora_detect_scan_acc_windows(plan._h, L, hop, acc) == Wa
    got = host(plan.scan_acc(torch.from_numpy(x[0]).cuda(), hop, acc))
    assert_bits(got, pc.scan_acc_host(O, x, sf, 1, hop, acc))


def test_no_window_two_strided_rows_and_an_odd_view(O, amd):
    sf, hop, step = 7, 32, 128
    plan = amd.DemodPlan(sf, dechirp=True, mode="raw")
    # W = 4 plain windows, none summed over two symbols
    short = torch.from_numpy(noise_rows(1, 2 * step - 1, 1)[0]).cuda()
    assert plan.scan_acc(short, hop, 2).power.shape == (1, 0)
    assert plan.scan_acc(short, hop, 1).power.shape == (1, 4)
    # two rows of a wider tensor: the samples behind a row are not its windows
    L = step * 3 + 5 * hop + 3
    x = noise_rows(2, L, 2)
    wide = torch.full((2, L + 37), 1e3 + 1e3j, dtype=torch.complex64, device="cuda")
    wide[:, :L] = torch.from_numpy(x).cuda()
    got = host(plan.scan_acc(wide[:, :L], hop, 2, conj=True))
    assert got["index"].shape == (2, 10)
    assert_bits(got, pc.scan_acc_host(O, x, sf, 1, hop, 2, True), "strided rows")
    # a view that begins 8 bytes into a larger tensor: the 16-byte loads need their guard
    big = torch.full((L + 11,), 1e3 - 1e3j, dtype=torch.complex64, device="cuda")
    big[3:3 + L] = torch.from_numpy(x[1]).cuda()
    got = host(plan.scan_acc(big[3:3 + L], hop, 2))
    assert_bits(got, pc.scan_acc_host(O, x[1], sf, 1, hop, 2), "odd view")
    # out=: written in place, columns beyond Wa left alone, an f_index refused
    want = pc.scan_acc_host(O, x[1], sf, 1, hop, 2)
    out = amd.DetectMetrics(torch.full((1, 13), 7.5, device="cuda"), torch.full((1, 13), 7.5, device="cuda"), None,
                            torch.full((1, 13), 0xABCD, dtype=torch.uint16, device="cuda"))
    assert plan.scan_acc(torch.from_numpy(x[1]).cuda(), hop, 2, out=out) is out
    got = host(out)
    assert_bits({k: v[:, :10] for k, v in got.items()}, want, "out=")
    assert (got["power"][:, 10:] == 7.5).all() and (got["index"][:, 10:] == 0xABCD).all()
    with pytest.raises(ValueError):
        plan.scan_acc(short, hop, 1, out=amd.DetectMetrics(*(torch.zeros((1, 4), device="cuda") for _ in range(3)),
                                                          torch.zeros((1, 4), dtype=torch.uint16, device="cuda")))
    with pytest.raises(ValueError):
        plan.scan_acc(short, 48, 2)  # acc > 1: hop must divide step
    with pytest.raises(ValueError):
        plan.scan_acc(short, hop, 9)
    assert plan.scan_acc(short, 48, 1).power.shape == (1, 3)


def test_capi_rules_with_a_plan(amd):
    """The entry's own refusals that read the plan's step, seen with a real plan; nothing runs."""
    from lora_phy_amd import _capi

    lib, E = _capi.lib(), _capi.LORA_EINVAL
    step, hop, L = 128, 32, 128 * 4
    plan = amd.DemodPlan(7, dechirp=True)
    h = plan._h
    assert lib.lora_detect_scan_acc_windows(h, L, hop, 1) == 13
    assert lib.lora_detect_scan_acc_windows(h, L, hop, 2) == 9 and lib.lora_detect_scan_acc_windows(h, L, hop, 4) == 1
    assert lib.lora_detect_scan_acc_windows(h, L, hop, 5) == 0
    assert lib.lora_detect_scan_acc_windows(h, L, 48, 1) == 9
    assert lib.lora_detect_scan_acc_windows(h, L, 48, 2) == E and "divide" in lib.lora_last_error().decode()
    assert lib.lora_detect_scan_acc_windows(h, L, hop, 0) == E and lib.lora_detect_scan_acc_windows(h, L, hop, 9) == E
    iq = torch.zeros(L, dtype=torch.complex64, device="cuda")
    buf = torch.full((16,), 3.0, device="cuda")

    def call(hop=hop, acc=2, ostride=9, iqp=iq.data_ptr(), power=buf.data_ptr()):
        return lib.lora_detect_scan_acc_batch(h, iqp, 1, L, L, hop, acc, 0, power, None, None, ostride, None)

    assert call(acc=0) == E and call(acc=9) == E
    assert call(hop=48) == E and "divide" in lib.lora_last_error().decode()
    assert call(ostride=8) == E and "out_stride" in lib.lora_last_error().decode()
    assert call(iqp=None) == E
    assert call(power=None, ostride=0) == 9  # no output: no launch, Wa returned
    torch.cuda.synchronize()
    assert (buf == 3.0).all()  # nothing ran
    assert call() == 9
    torch.cuda.synchronize()
    assert not (buf[:9] == 3.0).any() and (buf[9:] == 3.0).all()


def test_the_plain_scan_is_unchanged(O, amd):
    from tests import scan_checker as sc

    x, _, _ = sc.planted_stream(O, 7, 1, 6, (37, 5), 0.1, 0x12, 77)
    plan = amd.DemodPlan(7, dechirp=True, mode="raw")
    met = plan.scan(torch.from_numpy(x).cuda(), 32)
    torch.cuda.synchronize()
    want = sc.scan_host(O, x, 7, 1, 32, dechirp=True)
    for k in sc.FIELDS:
        g = getattr(met, k).cpu().numpy()
        assert np.array_equal(g if k == "index" else dc.bits(g), want[k] if k == "index" else dc.bits(want[k])), k
