"""GPU: the per-symbol detector metrics (k_detect_metrics behind lora_demod_metrics_batch,
DemodPlan.detect_metrics, LoRaDemod.work_metrics) against the reference's recorded detect()
outputs (tests/golden/detect_metrics.json) and the host checker (tests/detect_checker.py,
itself pinned to those records and to the oracle on the CPU).  Every float is compared by its
bit pattern: -inf, an exact 0 and the sign of a zero all count."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import detect_checker as dc
from tests.golden_inputs import STRESS, sha, stress_input

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIELDS = ("power", "power_avg", "f_index")


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


@pytest.fixture(scope="module")
def G():
    with open(os.path.join(GOLD, "golden.json")) as fh:
        return json.load(fh)


def host(met):
    torch.cuda.synchronize()
    return {k: getattr(met, k).cpu().numpy() for k in FIELDS + ("index",)}


def assert_bits(got, want, what=""):
    """got / want: dicts of [F, total] arrays; floats compared as bit patterns."""
    assert np.array_equal(got["index"], want["index"]), (what, "index")
    for k in FIELDS:
        g, w = dc.bits(got[k]), dc.bits(want[k])
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (what, k, len(bad), bad[:4].tolist(),
                               [(got[k][tuple(b)], want[k][tuple(b)]) for b in bad[:4]])


def sync_nibbles(index, sf):
    shift = max(sf - 4, 0)
    return (((index[:, 0].astype(int) >> shift) & 15) << 4) | ((index[:, 1].astype(int) >> shift) & 15)


def frames(O, sf, F, nsym, osr=1, bw=125000, amplitude=1.0, sigma=0.1, seed=1):
    """F noisy modulated frames of nsym data symbols; returns ([F, L] complex64, symbols)."""
    rng = np.random.default_rng(seed)
    syms = rng.integers(0, 1 << sf, (F, nsym)).astype(np.uint16)
    rows = []
    for f in range(F):
        x = O.lora_modulate(syms[f], sf, osr, bw, amplitude, 0x12)
        rows.append((x + sigma * (rng.standard_normal(len(x)) + 1j * rng.standard_normal(len(x)))).astype(np.complex64))
    return np.stack(rows), syms


def run_legacy(amd, O, x, sf, osr=1, hann=False, dech=False, bw=125000, pipeline=None, mode="legacy"):
    """run + detect_metrics on the GPU and the checker on the run's own per-frame outputs."""
    plan = amd.DemodPlan(sf, osr, bw, "hann" if hann else "none", dechirp=dech, mode=mode, pipeline=pipeline)
    xt = torch.from_numpy(x).cuda()
    res = plan.run(xt)
    got = host(plan.detect_metrics(xt, res))
    want = dc.frames_metrics(O, x, sf, osr, mode, hann, dech, bw, res.cfo.cpu().numpy(),
                             res.time_offset.cpu().numpy(), res.max_amp.cpu().numpy())
    return res, got, want


# ---- the reference's recorded outputs ------------------------------------------------------
@pytest.mark.parametrize("sf", dc.GOLDEN_SFS)
def test_reference_records_through_a_raw_plan(amd, O, sf):
    """The fixture windows of one SF, one per frame of one batch, through a RAW plan with no
    dechirp and no window: the outputs equal the bits the reference's compiled detect() gave,
    the -inf / exact-0 edge rows and both wrap-around neighbours included."""
    with open(os.path.join(GOLD, "detect_metrics.json")) as fh:
        recs = [r for r in json.load(fh)["records"] if r["sf"] == sf]
    wins = dc.golden_windows(O, sf)
    assert [r["name"] for r in recs] == [n for n, _ in wins] and len(recs) >= 12
    for r, (_, w) in zip(recs, wins):
        assert sha(w) == r["sha256"]
    names = {r["name"] for r in recs}
    assert {"zero", "constant", "alternating", "clean_0", "clean_last"} <= names
    plan = amd.DemodPlan(sf, mode="raw")
    got = host(plan.detect_metrics(torch.from_numpy(np.stack([w for _, w in wins])).cuda()))
    want = {"index": np.array([[r["index"]] for r in recs], np.uint16)}
    for k in FIELDS:
        want[k] = np.array([[r[k]] for r in recs], np.uint32).view(np.float32)
    assert_bits(got, want, f"SF{sf}")


# ---- LEGACY against the checker -------------------------------------------------------------
@pytest.mark.parametrize("ci", range(len(STRESS)))
def test_stress_cases_legacy(G, O, amd, ci):
    """Every STRESS case (SF 2-12, osr 1-4, both windows, dechirp on / off, both t_off signs,
    scaled / unscaled, frames of one and of no whole symbol): run, then detect_metrics."""
    case = STRESS[ci]
    sf, osr, hann, dech, F = case[:5]
    x = stress_input(O, case, G["stress"][ci]["seed"])
    assert sha(x) == G["stress"][ci]["iq_sha256"]
    res, got, want = run_legacy(amd, O, x, sf, osr, hann, dech)
    total = x.shape[1] // ((1 << sf) * osr)
    assert got["index"].shape == (F, total)
    assert_bits(got, want, f"case {ci}")
    syms = res.symbols.cpu().numpy()
    if total >= 2:
        assert np.array_equal(got["index"][:, 2:], syms)
        assert np.array_equal(sync_nibbles(got["index"], sf), res.sync.cpu().numpy().astype(int))
    else:
        assert np.array_equal(got["index"], syms)


def test_both_pipelines_feed_the_same_metrics(G, O, amd):
    case = STRESS[5]  # SF7, 66 symbols, fused dechirp: the speculative pipeline's shape
    x = stress_input(O, case, G["stress"][5]["seed"])
    out = {}
    for pipe in ("spec", "split"):
        plan = amd.DemodPlan(7, dechirp=True, pipeline=pipe)
        xt = torch.from_numpy(x).cuda()
        res = plan.run(xt)
        assert ("spec" in plan.last_kernels()) == (pipe == "spec")
        out[pipe] = host(plan.detect_metrics(xt, res))
    assert_bits(out["spec"], out["split"])


@pytest.mark.parametrize("amplitude", [2.5, 0.5])
@pytest.mark.parametrize("sf,F", [(7, 1), (7, 3), (7, 65), (10, 1), (10, 3), (10, 65)])
def test_legacy_scaled_and_unscaled(O, amd, sf, F, amplitude):
    """5 data symbols per frame, so the symbol counts do not fill the last workgroup.  The 65
    frames are drawn (seeded, irregularly) from 6 distinct ones, which keeps the host checker
    to 6 frames while every frame and workgroup boundary is still checked."""
    base, _ = frames(O, sf, min(F, 6), 5, amplitude=amplitude, sigma=0.05, seed=sf * 100 + F)
    pick = np.random.default_rng(F).integers(0, len(base), F) if F > len(base) else np.arange(F)
    x = base[pick]
    plan = amd.DemodPlan(sf, dechirp=True)
    xt = torch.from_numpy(x).cuda()
    res = plan.run(xt)
    amp = res.max_amp.cpu().numpy()
    assert (amp > 1.0).all() if amplitude > 1 else (amp <= 1.0).all()
    got = host(plan.detect_metrics(xt, res))
    sel = [int(np.flatnonzero(pick == b)[0]) for b in range(len(base))]
    wb = dc.frames_metrics(O, base, sf, 1, "legacy", False, True, 125000, res.cfo.cpu().numpy()[sel],
                           res.time_offset.cpu().numpy()[sel], amp[sel])
    assert_bits(got, {k: v[pick] for k, v in wb.items()}, f"SF{sf} F{F}")
    assert np.array_equal(got["index"][:, 2:], res.symbols.cpu().numpy())


def test_bw500_sf9_legacy(O, amd):
    x, _ = frames(O, 9, 2, 4, bw=500000, seed=9)
    res, got, want = run_legacy(amd, O, x, 9, dech=True, bw=500000)
    assert_bits(got, want)
    assert np.array_equal(got["index"][:, 2:], res.symbols.cpu().numpy())


def test_hand_made_offsets_check_the_guards_and_the_rotation(O, amd):
    """time_offset in {+-0.5, 2.5, +-(N osr + 3)} and beyond int (saturating; NaN gives 0) with
    non-zero cfo, per frame, against the checker: the base guards of LoRaDemod.cpp:143-149,
    half-away rounding, the dechirp-table phase of a shifted window and the rotation."""
    sf, osr = 7, 2
    step = (1 << sf) * osr
    toff = np.array([0.5, -0.5, 2.5, step + 3, -(step + 3), float("nan"), 3e9, -3e9, -1.49], np.float32)
    F = len(toff)
    x, _ = frames(O, sf, F, 5, osr=osr, amplitude=1.5, sigma=0.1, seed=77)
    x = np.ascontiguousarray(x[:, :-5])  # a ragged tail: the last window's positive shift is refused
    cfo = np.linspace(-0.3, 0.4, F).astype(np.float32)
    amp = np.where(np.arange(F) % 2 == 0, 2.0, 0.75).astype(np.float32)
    plan = amd.DemodPlan(sf, osr, window="hann", dechirp=True)
    res = amd.DemodResult(None, None, torch.from_numpy(cfo).cuda(), torch.from_numpy(toff).cuda(),
                          torch.from_numpy(amp).cuda())
    got = host(plan.detect_metrics(torch.from_numpy(x).cuda(), res))
    want = dc.frames_metrics(O, x, sf, osr, "legacy", True, True, 125000, cfo, toff, amp)
    assert_bits(got, want)


# ---- API and RAW ---------------------------------------------------------------------------
@pytest.mark.parametrize("osr,hann", [(1, False), (1, True), (2, False), (2, True)])
def test_api_mode(O, amd, osr, hann):
    x, _ = frames(O, 7, 3, 6, osr=osr, sigma=0.25, seed=40 + osr)
    res, got, want = run_legacy(amd, O, x, 7, osr, hann, mode="api")
    assert_bits(got, want)
    assert np.array_equal(got["index"][:, 2:], res.symbols.cpu().numpy())
    assert np.array_equal(sync_nibbles(got["index"], 7), res.sync.cpu().numpy().astype(int))


@pytest.mark.parametrize("sf", [7, 9])
def test_raw_with_dechirp_hann_osr2(O, amd, sf):
    x, _ = frames(O, sf, 2, 3, osr=2, sigma=0.2, seed=sf)
    plan = amd.DemodPlan(sf, 2, window="hann", dechirp=True, mode="raw")
    xt = torch.from_numpy(x).cuda()
    got = host(plan.detect_metrics(xt))  # no result needed
    assert_bits(got, dc.frames_metrics(O, x, sf, 2, "raw", True, True))
    assert np.array_equal(got["index"], plan.run(xt).symbols.cpu().numpy())


# ---- layout, the C-ABI's rules, graphs, the Python surface -----------------------------------
def test_layout_strides_sentinels_and_single_outputs(O, amd):
    sf, F = 7, 5
    x, _ = frames(O, sf, F, 4, sigma=0.1, seed=5)
    L, total = x.shape[1], x.shape[1] >> sf
    plan = amd.DemodPlan(sf, dechirp=True)
    xt = torch.from_numpy(x).cuda()
    res = plan.run(xt)
    ref = host(plan.detect_metrics(xt, res))
    # row-strided input, outputs wider than total: the columns beyond keep the sentinel
    wide = torch.zeros((F, L + 37), dtype=torch.complex64, device="cuda")
    wide[:, :L] = xt
    res_w = plan.run(wide[:, :L])
    W = total + 3
    out = amd.DetectMetrics(*(torch.full((F, W), 7.5, device="cuda") for _ in range(3)),
                            torch.full((F, W), 0xABCD, dtype=torch.uint16, device="cuda"))
    assert plan.detect_metrics(wide[:, :L], res_w, out=out) is out
    got = host(out)
    assert_bits({k: v[:, :total] for k, v in got.items()}, ref)
    for k in FIELDS:
        assert (got[k][:, total:] == 7.5).all()
    assert (got["index"][:, total:] == 0xABCD).all()
    # the same tensors again (reused), after a change of input
    xt2 = xt.flip(0).contiguous()
    res2 = plan.run(xt2)
    assert_bits({k: v[:, :total] for k, v in host(plan.detect_metrics(xt2, res2, out=out)).items()},
                {k: v[::-1] for k, v in ref.items()})
    # each output alone, the others NULL
    for k, dt in (("power", torch.float32), ("power_avg", torch.float32), ("f_index", torch.float32),
                  ("index", torch.uint16)):
        one = amd.DetectMetrics(None, None, None, None)
        setattr(one, k, torch.zeros((F, total), dtype=dt, device="cuda"))
        plan.detect_metrics(xt, res, out=one)
        torch.cuda.synchronize()
        g = getattr(one, k).cpu().numpy()
        assert np.array_equal(g if k == "index" else dc.bits(g), ref[k] if k == "index" else dc.bits(ref[k])), k
    # a single [L] frame
    one = host(plan.detect_metrics(xt[0], amd.DemodResult(None, None, res.cfo[:1], res.time_offset[:1], res.max_amp[:1])))
    assert_bits(one, {k: v[:1] for k, v in ref.items()})
    with pytest.raises(ValueError):
        plan.detect_metrics(xt)  # a legacy plan needs result=
    with pytest.raises(ValueError):
        plan.detect_metrics(xt, res, out=amd.DetectMetrics(torch.zeros((F, total - 1), device="cuda"), None, None, None))
    with pytest.raises(TypeError):
        plan.detect_metrics(xt, res, out=amd.DetectMetrics(torch.zeros((F, total), dtype=torch.float64, device="cuda"),
                                                           None, None, None))


def test_capi_rules_with_a_plan(amd):
    from lora_phy_amd import _capi

    lib = _capi.lib()
    N, F, total = 128, 2, 3
    L = total * N
    iq = torch.zeros((F, L), dtype=torch.complex64, device="cuda")
    v = torch.zeros(F, device="cuda")
    buf = torch.full((F, total), 3.0, device="cuda")
    legacy, api, raw = amd.DemodPlan(7), amd.DemodPlan(7, mode="api"), amd.DemodPlan(7, mode="raw")

    def call(plan, frames=F, frame_len=L, stride=L, cfo=v, toff=v, amp=v, ostride=total, iqp=iq, power=buf):
        m = _capi.SymbolMetrics(power.data_ptr() if power is not None else None, None, None, None, ostride)
        return lib.lora_demod_metrics_batch(plan._h, iqp.data_ptr() if iqp is not None else None, frames, frame_len,
                                            stride, *(t.data_ptr() if t is not None else None for t in (cfo, toff, amp)),
                                            C.byref(m), None)

    E = _capi.LORA_EINVAL
    assert call(legacy, iqp=None) == E and lib.lora_last_error().decode()
    assert call(legacy, frames=-1) == E
    assert call(legacy, frame_len=-1) == E
    assert call(legacy, stride=L - 1) == E
    assert call(legacy, ostride=total - 1) == E
    assert call(legacy, cfo=None) == E and call(legacy, toff=None) == E and call(legacy, amp=None) == E
    assert call(api, cfo=None) == E and call(api, toff=None) == E
    assert call(api, frame_len=L - 1) == E and call(api, frame_len=N, stride=N) == E  # the plan's own rule
    torch.cuda.synchronize()
    assert (buf == 3.0).all()  # nothing ran
    # no launch: frames == 0 (buffers may be NULL), total == 0, no output given - all return total
    assert call(legacy, frames=0, iqp=None, cfo=None, toff=None, amp=None) == total
    assert call(legacy, frame_len=N - 1, stride=N - 1) == 0
    assert call(legacy, power=None, ostride=0) == total
    torch.cuda.synchronize()
    assert (buf == 3.0).all()
    # what may be NULL: max_amp in API, all three in RAW; one frame with any frame_stride
    assert call(api, amp=None) == total
    assert call(raw, cfo=None, toff=None, amp=None) == total
    assert call(raw, frames=1, stride=0, cfo=None, toff=None, amp=None) == total
    torch.cuda.synchronize()
    # zero frames through the Python surface
    met = raw.detect_metrics(torch.zeros((0, L), dtype=torch.complex64, device="cuda"))
    assert met.power.shape == (0, total) and met.index.dtype == torch.uint16


def test_graph_capture_and_replay(O, amd):
    x, _ = frames(O, 7, 4, 5, sigma=0.2, seed=11)
    x2, _ = frames(O, 7, 4, 5, sigma=0.4, seed=12)
    plan = amd.DemodPlan(7, dechirp=True)
    xt = torch.from_numpy(x).cuda()
    res = plan.run(xt)
    out = plan.detect_metrics(xt, res)
    eager = host(out)
    xt2 = torch.from_numpy(x2).cuda()
    res2 = plan.run(xt2)
    eager2 = host(plan.detect_metrics(xt2, res2))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        plan.detect_metrics(xt, res, out=out)
    torch.cuda.current_stream().wait_stream(s)
    for t in (out.power, out.power_avg, out.f_index, out.index):
        t.zero_()
    with torch.cuda.graph(g):
        plan.detect_metrics(xt, res, out=out)
    g.replay()
    assert_bits(host(out), eager)
    xt.copy_(xt2)  # new frames and offsets in the captured buffers
    for a, b in ((res.cfo, res2.cfo), (res.time_offset, res2.time_offset), (res.max_amp, res2.max_amp)):
        a.copy_(b)
    g.replay()
    assert_bits(host(out), eager2)


def test_snr_helpers_and_work_metrics(O, amd):
    x, _ = frames(O, 8, 3, 6, sigma=0.3, seed=21)
    xt = torch.from_numpy(x).cuda()
    demod = amd.LoRaDemod(8)
    met = demod.work_metrics(xt)
    assert demod.last is not None and demod.last.symbols.shape == (3, 6)
    plan = amd.DemodPlan(8, dechirp=True)
    res = plan.run(xt)
    assert_bits(host(met), host(plan.detect_metrics(xt, res)))
    assert np.array_equal(demod.last.symbols.cpu().numpy(), res.symbols.cpu().numpy())
    h = host(met)
    snr = met.snr_db.cpu().numpy()
    assert np.array_equal(dc.bits(snr), dc.bits(h["power"] - h["power_avg"]))
    assert (snr[:, 2:] > 3.0).all()  # tones well above the floor
    for first in (2, 0):
        want = (h["power"] - h["power_avg"])[:, first:].astype(np.float64).mean(axis=1).astype(np.float32)
        assert np.array_equal(dc.bits(met.frame_snr_db(first).cpu().numpy()), dc.bits(want))
    # a floor of -inf stays +inf
    ones = torch.ones((1, 256), dtype=torch.complex64, device="cuda")
    raw = amd.DemodPlan(8, mode="raw").detect_metrics(ones)
    assert raw.snr_db.cpu().numpy()[0, 0] == np.inf and raw.frame_snr_db(0).cpu().numpy()[0] == np.inf
