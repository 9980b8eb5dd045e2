"""GPU: the soft-decision receive path - k_soft_bits behind lora_demod_soft_bits_batch and
DemodPlan.soft_bits, k_soft_chain_decode behind lora_decode_chain_soft_batch and
codec.decode_chain_soft, LoRaDemod.work_payload_soft - against the host checker
(tests/soft_checker.py, itself checked on the CPU by tests/test_soft_checker.py).  Every float
is compared by its bit pattern, payloads and counts exactly."""
import numpy as np
import pytest

from lora_phy_amd import codes
from tests import detect_checker as dc
from tests import soft_checker as sc

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


def frames(O, sf, F, nsym, sigmas, osr=1, bw=125000, amplitude=1.0, seed=1):
    """F modulated frames of nsym data symbols, row f with noise sigmas[f % len] per component
    (None = an all-zero row)."""
    rng = np.random.default_rng(seed)
    rows = []
    for f in range(F):
        x = O.lora_modulate(rng.integers(0, 1 << sf, nsym).astype(np.uint16), sf, osr, bw, amplitude, 0x12)
        s = sigmas[f % len(sigmas)]
        n = rng.standard_normal(len(x)) + 1j * rng.standard_normal(len(x))
        rows.append(np.zeros(len(x), np.complex64) if s is None else (x + s * n).astype(np.complex64))
    return np.stack(rows)


def assert_llr_bits(got, want, what=""):
    g, w = dc.bits(got), dc.bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.argwhere(g != w)
    assert len(bad) == 0, (what, len(bad), bad[:4].tolist(), [(got[tuple(b)], want[tuple(b)]) for b in bad[:4]])


def run_soft(amd, O, x, sf, osr=1, hann=False, dech=False, bw=125000, mode="legacy", xt=None):
    """run + soft_bits on the GPU and the checker on the run's own per-frame outputs."""
    plan = amd.DemodPlan(sf, osr, bw, "hann" if hann else "none", dechirp=dech, mode=mode)
    xt = torch.from_numpy(x).cuda() if xt is None else xt
    res = plan.run(xt)
    got = plan.soft_bits(xt, res)
    torch.cuda.synchronize()
    want = sc.soft_bits_frames(O, x, sf, osr, mode, hann, dech, bw, res.cfo.cpu().numpy(),
                               res.time_offset.cpu().numpy(), res.max_amp.cpu().numpy())
    return plan, res, got, want


# ---- soft_bits against the checker -----------------------------------------------------------
@pytest.mark.parametrize("F", [5, 30])
def test_sf6_partial_and_crossing_groups(O, amd, F):
    """G = 64 symbols per workgroup: 5 frames of 2 + 3 symbols are 15 work items (one partial
    group); 30 frames are 150 (groups that cross frames, frames that cross groups).  The 30
    are drawn from 6 distinct ones, which keeps the host checker to 6 frames."""
    base = frames(O, 6, min(F, 6), 3, [0.3, 0.05, 1.0], seed=60 + F)
    pick = np.random.default_rng(F).integers(0, len(base), F) if F > len(base) else np.arange(F)
    pick[:len(base)] = np.arange(len(base))
    x = base[pick]
    plan = amd.DemodPlan(6, dechirp=True)
    xt = torch.from_numpy(x).cuda()
    res = plan.run(xt)
    got = plan.soft_bits(xt, res).cpu().numpy()
    assert got.shape == (F, 5, 6) and got.dtype == np.float32
    n = len(base)
    want = sc.soft_bits_frames(O, base, 6, 1, "legacy", False, True, 125000, res.cfo.cpu().numpy()[:n],
                               res.time_offset.cpu().numpy()[:n], res.max_amp.cpu().numpy()[:n])
    assert_llr_bits(got, want[pick], f"SF6 F{F}")


SF7_SIGMAS = [0.0, 10.0 ** (0 / 20.0), 10.0 ** (10 / 20.0), None]  # noiseless, 0 dB, -10 dB, all-zero


@pytest.fixture(scope="module")
def sf7_cases(O, amd):
    """SF 7 (G = 32), 7 frames of 2 + 5 symbols with noiseless, 0 dB, -10 dB and one all-zero
    row mixed in one batch, in the three modes: (name, sf, iq, llr on the GPU, checker's)."""
    out = []
    for name, kw in (("legacy", dict(dech=True)), ("api", dict(mode="api")),
                     ("raw", dict(mode="raw", hann=True, dech=True, osr=2, bw=250000))):
        x = frames(O, 7, 7, 5, SF7_SIGMAS, osr=kw.get("osr", 1), bw=kw.get("bw", 125000), seed=70)
        plan, res, got, want = run_soft(amd, O, x, 7, **kw)
        out.append((name, x, plan, res, got, want))
    return out


def test_sf7_three_modes_mixed_rows(sf7_cases):
    for name, x, plan, res, got, want in sf7_cases:
        g = got.cpu().numpy()
        assert g.shape == (7, 7, 7)
        assert_llr_bits(g, want, name)
        assert (dc.bits(g[3]) == 0).all(), name  # the all-zero frame: every LLR is +0.0
        assert not np.isnan(g).any()


def test_sf7_signs_are_the_demodulated_symbols(sf7_cases):
    """Wherever llr != 0 its sign is the bit of grayToBinary16 of the symbol run() returned."""
    for name, x, plan, res, got, want in sf7_cases:
        g = got.cpu().numpy()
        syms = res.symbols.cpu().numpy()
        data = g[:, 2:] if name != "raw" else g
        v = codes.gray_to_binary16(syms).astype(np.int64)
        bit = (v[:, :, None] >> np.arange(7)[None, None, :]) & 1
        nz = data != 0
        assert np.array_equal((data > 0)[nz], bit[nz] == 1), name


def test_out_tensor_pitch_spare_rows_and_sentinel(sf7_cases, amd):
    name, x, plan, res, got, want = sf7_cases[0]
    xt = torch.from_numpy(x).cuda()
    F, total, sf = 7, 7, 7
    out = torch.full((F + 2, total + 3, sf), -7.5, device="cuda")
    view = plan.soft_bits(xt, res, out=out)
    assert view.data_ptr() == out.data_ptr() and view.shape == (F, total, sf)
    o = out.cpu().numpy()
    assert_llr_bits(o[:F, :total], want)
    assert (o[F:] == -7.5).all() and (o[:, total:] == -7.5).all()
    # a single [L] frame, and what the wrapper refuses
    one = plan.soft_bits(xt[1], amd.DemodResult(None, None, res.cfo[1:2], res.time_offset[1:2], res.max_amp[1:2]))
    assert_llr_bits(one.cpu().numpy(), want[1:2])
    with pytest.raises(ValueError):
        plan.soft_bits(xt)  # a legacy plan needs result=
    with pytest.raises(ValueError):
        plan.soft_bits(xt, res, out=torch.zeros((F, total - 1, sf), device="cuda"))
    with pytest.raises(ValueError):
        plan.soft_bits(xt, res, out=torch.zeros((F, total, sf + 1), device="cuda")[:, :, :sf])
    with pytest.raises(TypeError):
        plan.soft_bits(xt, res, out=torch.zeros((F, total, sf), dtype=torch.float64, device="cuda"))


@pytest.fixture(scope="module")
def sf9_case(O, amd):
    """SF 9 (G = 8), 3 frames of 2 + 4 symbols, the rows a strided view with a gap."""
    x = frames(O, 9, 3, 4, [0.5, 2.0, 0.1], seed=90)
    L = x.shape[1]
    wide = torch.zeros((3, L + 131), dtype=torch.complex64, device="cuda")
    wide[:, :L] = torch.from_numpy(x).cuda()
    return (x,) + run_soft(amd, O, x, 9, dech=True, xt=wide[:, :L])


def test_sf9_strided_rows(sf9_case):
    x, plan, res, got, want = sf9_case
    assert_llr_bits(got.cpu().numpy(), want, "SF9")


def test_sf12_one_frame(O, amd):
    """SF 12: G = 1, the symbol spans the four waves, bits 6-11 are uniform over a wave."""
    x = frames(O, 12, 1, 2, [3.0], seed=120)
    plan, res, got, want = run_soft(amd, O, x, 12, dech=True)
    assert got.shape == (1, 4, 12)
    assert_llr_bits(got.cpu().numpy(), want, "SF12")


def test_capi_rules_with_a_plan(amd):
    from lora_phy_amd import _capi

    lib = _capi.lib()
    N, F, total, sf = 128, 2, 3, 7
    L = total * N
    iq = torch.zeros((F, L), dtype=torch.complex64, device="cuda")
    v = torch.zeros(F, device="cuda")
    buf = torch.full((F, total, sf), 3.0, device="cuda")
    legacy, api, raw = amd.DemodPlan(7), amd.DemodPlan(7, mode="api"), amd.DemodPlan(7, mode="raw")
    sf5 = amd.DemodPlan(5, mode="raw")

    def call(plan, frames=F, frame_len=L, stride=L, cfo=v, toff=v, amp=v, lstride=total, iqp=iq, llr=buf):
        return lib.lora_demod_soft_bits_batch(plan._h, iqp.data_ptr() if iqp is not None else None, frames, frame_len,
                                              stride, *(t.data_ptr() if t is not None else None for t in (cfo, toff, amp)),
                                              llr.data_ptr() if llr is not None else None, lstride, None)

    E = _capi.LORA_EINVAL
    assert call(legacy, iqp=None) == E and lib.lora_last_error().decode()
    assert call(legacy, frames=-1) == E and call(legacy, frame_len=-1) == E and call(legacy, stride=L - 1) == E
    assert call(legacy, lstride=total - 1) == E and call(legacy, lstride=-1) == E
    assert call(legacy, cfo=None) == E and call(legacy, toff=None) == E and call(legacy, amp=None) == E
    assert call(api, cfo=None) == E and call(api, toff=None) == E
    assert call(api, frame_len=L - 1) == E and call(api, frame_len=N, stride=N) == E  # the plan's own rule
    assert call(sf5, frame_len=96, stride=96, cfo=None, toff=None, amp=None) == E  # sf < 6
    torch.cuda.synchronize()
    assert (buf == 3.0).all()  # nothing ran
    # no launch: frames == 0 (buffers may be NULL), total == 0, a NULL llr - all return total
    assert call(legacy, frames=0, iqp=None, cfo=None, toff=None, amp=None) == total
    assert call(legacy, frame_len=N - 1, stride=N - 1) == 0
    assert call(legacy, llr=None, lstride=0) == total
    torch.cuda.synchronize()
    assert (buf == 3.0).all()
    assert call(api, amp=None) == total
    assert call(raw, cfo=None, toff=None, amp=None) == total
    torch.cuda.synchronize()
    assert (dc.bits(buf.cpu().numpy()) == 0).all()  # zero frames: every LLR +0.0
    with pytest.raises(ValueError):
        sf5.soft_bits(torch.zeros((1, 96), dtype=torch.complex64, device="cuda"))
    got = raw.soft_bits(torch.zeros((0, L), dtype=torch.complex64, device="cuda"))
    assert got.shape == (0, total, sf) and got.dtype == torch.float32


# ---- decode_chain_soft against the checker ---------------------------------------------------
def synthetic_llrs(rng, F, S, sf, rdd):
    """Seeded standard-normal LLRs with a sprinkling of +-0.0, exact ties (two equal magnitudes
    in a codeword), +-inf and NaN."""
    a = rng.standard_normal((F, S, sf)).astype(np.float32)
    nb = 4 + rdd
    flat = a.reshape(-1)
    for val in (0.0, -0.0, np.inf, -np.inf, np.nan):
        flat[rng.integers(0, flat.size, max(1, flat.size // 97))] = np.float32(val)
    for f in range(F):  # ties: bits 0 and 1 of a codeword get the same magnitude
        for blk in range(S // nb):
            dst = int(rng.integers(0, sf))
            a[f, blk * nb + 1, (dst - 1) % sf] = -a[f, blk * nb, dst]
    return a


def check_decode(amd, llr_t, llr_np, sf, rdd, nbytes, what):
    res = amd.codec.decode_chain_soft(llr_t, sf, rdd, nbytes)
    torch.cuda.synchronize()
    pay, corr = sc.decode_chain_soft_frames(llr_np, sf, rdd, nbytes)
    assert res.crc_ok is None and res.bad is None
    assert np.array_equal(res.payload.cpu().numpy(), pay), what
    assert np.array_equal(res.errors.cpu().numpy(), corr), what


@pytest.mark.parametrize("rdd", range(5))
@pytest.mark.parametrize("sf", range(6, 13))
def test_decode_chain_soft_synthetic(amd, sf, rdd):
    rng = np.random.default_rng(1000 * sf + rdd)
    nb = 4 + rdd
    odd = 11  # 22 codewords: a partial last block at every sf
    for nbytes, F, view in ((0, 5, False), (1, 257, True), (odd, 5, False), (255, 1, False), (odd, 1, True)):
        S = -(-2 * nbytes // sf) * nb + (3 if nbytes else nb)  # whole blocks plus trailing symbols
        a = synthetic_llrs(rng, F, S + (2 if view else 0), sf, rdd)
        t = torch.from_numpy(a).cuda()
        if view:
            t, a = t[:, 2:], a[:, 2:]
        check_decode(amd, t, a, sf, rdd, nbytes, (sf, rdd, nbytes, F, view))
    # a single [S, sf] frame, outputs given
    a = synthetic_llrs(rng, 1, 2 * nb, sf, rdd)
    n = 2 * sf // 2
    out = amd.codec.DecodeResult(torch.zeros(n, dtype=torch.uint8, device="cuda"), None,
                                 torch.full((1,), -1, dtype=torch.int32, device="cuda"), None)
    assert amd.codec.decode_chain_soft(torch.from_numpy(a[0]).cuda(), sf, rdd, n, out=out) is out
    pay, corr = sc.decode_chain_soft(a[0], sf, rdd, n)
    assert np.array_equal(out.payload.cpu().numpy(), pay) and int(out.errors[0]) == corr


def test_decode_chain_soft_wrapper_rules(amd):
    t = torch.zeros((2, 10, 7), device="cuda")
    with pytest.raises(TypeError):
        amd.codec.decode_chain_soft(t.double(), 7, 1, 3)
    with pytest.raises(ValueError):
        amd.codec.decode_chain_soft(t, 8, 1, 3)  # last dimension is not sf
    with pytest.raises(ValueError):
        amd.codec.decode_chain_soft(t[:, :, ::2], 4, 1, 3)
    with pytest.raises(ValueError):
        amd.codec.decode_chain_soft(t, 7, 1, 256)
    with pytest.raises(amd._capi.LoraError) as e:
        amd.codec.decode_chain_soft(t, 7, 1, 8)  # two blocks carry 14 codewords
    assert e.value.code == amd._capi.LORA_ERANGE


def test_decode_on_the_llrs_soft_bits_produced(sf7_cases, sf9_case, amd):
    for name, x, plan, res, got, want in sf7_cases:
        data_t, data = (got[:, 2:], want[:, 2:]) if name != "raw" else (got, want)
        for rdd in (1, 4):
            nbytes = data.shape[1] // (4 + rdd) * 7 // 2
            check_decode(amd, data_t, data, 7, rdd, nbytes, (name, rdd))
    x, plan, res, got, want = sf9_case
    check_decode(amd, got[:, 2:], want[:, 2:], 9, 0, 4, "SF9")


# ---- end to end ------------------------------------------------------------------------------
def test_end_to_end_work_payload_soft(O, amd):
    """LoRaMod.work_payload(chain="lora") -> host-generated seeded noise, SF 7, CR 4/5, -7 dB
    (soft_checker.noise_sigma), 64 frames of 16 bytes -> LoRaDemod.work_payload_soft."""
    sf, cr, F, nbytes = 7, 1, 64, 16
    rng = np.random.default_rng(77)
    pay = rng.integers(0, 256, (F, nbytes)).astype(np.uint8)
    clean = amd.LoRaMod(sf, cr=cr).work_payload(torch.from_numpy(pay), chain="lora")
    demod = amd.LoRaDemod(sf, cr=cr)
    quiet = demod.work_payload_soft(clean, nbytes)
    assert np.array_equal(quiet.payload.cpu().numpy(), pay) and int(quiet.errors.abs().sum()) == 0
    s = sc.noise_sigma(-7.0)
    noise = (s * (rng.standard_normal(clean.shape) + 1j * rng.standard_normal(clean.shape))).astype(np.complex64)
    iq = clean + torch.from_numpy(noise).cuda()
    soft = demod.work_payload_soft(iq, nbytes)
    res = demod.last
    assert res.symbols.shape == (F, 25)
    hard = demod.work_payload(iq, nbytes, chain="lora")
    x = iq.cpu().numpy()
    want = sc.soft_bits_frames(O, x, sf, 1, "legacy", False, True, 125000, res.cfo.cpu().numpy(),
                               res.time_offset.cpu().numpy(), res.max_amp.cpu().numpy())
    wpay, wcorr = sc.decode_chain_soft_frames(want[:, 2:], sf, cr, nbytes)
    got = soft.payload.cpu().numpy()
    assert np.array_equal(got, wpay)
    assert np.array_equal(soft.errors.cpu().numpy(), wcorr)
    soft_bad = int((got != pay).any(axis=1).sum())
    hard_bad = int((hard.payload.cpu().numpy() != pay).any(axis=1).sum())
    print(f"wrong frames of {F}: hard {hard_bad}, soft {soft_bad}")
    assert soft_bad <= hard_bad
    # default nbytes: what the whole blocks carry; a single [L] frame
    assert demod.work_payload_soft(iq).payload.shape == (F, 17)
    one = demod.work_payload_soft(iq[3], nbytes)
    assert one.payload.shape == (nbytes,) and np.array_equal(one.payload.cpu().numpy(), wpay[3])


# ---- HIP graph -------------------------------------------------------------------------------
def test_graph_capture_of_run_soft_bits_and_decode(O, amd):
    sf, rdd, nbytes, F = 7, 1, 7, 4
    rng = np.random.default_rng(5)
    pays = rng.integers(0, 256, (2, F, nbytes)).astype(np.uint8)
    xs = [sc.chain_frames(O, sf, rdd, p, snr, rng) for p, snr in zip(pays, (-2.0, -6.0))]
    plan = amd.DemodPlan(sf, dechirp=True)
    x = torch.from_numpy(xs[0]).cuda()
    total = x.shape[1] >> sf
    eager = []
    for xa in xs:
        xt = torch.from_numpy(xa).cuda()
        r = plan.run(xt)
        d = amd.codec.decode_chain_soft(plan.soft_bits(xt, r)[:, 2:], sf, rdd, nbytes)
        torch.cuda.synchronize()
        eager.append((dc.bits(plan.soft_bits(xt, r).cpu().numpy()), d.payload.cpu().numpy(), d.errors.cpu().numpy()))
    res = plan.run(x)
    llr = torch.zeros((F, total, sf), device="cuda")
    dec = amd.codec.DecodeResult(torch.zeros((F, nbytes), dtype=torch.uint8, device="cuda"), None,
                                 torch.zeros(F, dtype=torch.int32, device="cuda"), None)

    def chain():
        plan.run(x, out=res)
        plan.soft_bits(x, res, out=llr)
        amd.codec.decode_chain_soft(llr[:, 2:], sf, rdd, nbytes, out=dec)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        chain()  # warm-up on a side stream: workspaces exist before the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain()
    for xa, (ebits, epay, eerr) in zip(reversed(xs), reversed(eager)):
        x.copy_(torch.from_numpy(xa).cuda())
        llr.fill_(-1.0)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(dc.bits(llr.cpu().numpy()), ebits)
        assert np.array_equal(dec.payload.cpu().numpy(), epay) and np.array_equal(dec.errors.cpu().numpy(), eerr)
