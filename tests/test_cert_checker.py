"""CPU: the premises of the certification bound that the reference alone decides, and the host
model tests/cert_checker.py that tests/test_gpu_cert.py holds the kernels to.

* The reference's share of the bound: every bin of the oracle's fp32 transform (kissfft order)
  lies within E sum|y_i| of the float64 one, E = (8 SF + 42) 2^-24, with and without Hann.
* The margin model picks the oracle's bin wherever its margin exceeds twice that error.
* Each variant's near-tie sweep holds, by the reference data alone, symbols the criterion
  certifies and symbols it rejects, so the GPU comparison cannot pass vacuously.
* Each LEGACY variant's noiseless offsets batch holds a frame whose pre-pass and exact time
  offsets differ by the oracle, so the whole-frame rejection is driven too.
"""
import numpy as np
import pytest

from tests import cert_checker as cc


@pytest.fixture(scope="module")
def O():
    from oracle.pyoracle import Oracle

    return Oracle()


@pytest.mark.parametrize("hann", [False, True])
@pytest.mark.parametrize("sf", [6, 7, 8, 9, 10, 11, 12])
def test_reference_transform_stays_within_its_share_of_the_bound(O, sf, hann):
    worst = cc.reference_share(O, sf, hann)
    print(f"REFERENCE_SHARE sf={sf} hann={hann}: worst |X32 - X64| / (E sum|y|) = {worst:.4f}")
    assert worst <= 1.0


@pytest.mark.parametrize("hann", [False, True])
@pytest.mark.parametrize("sf", [6, 7, 9, 10, 12])
def test_margin_model_picks_the_oracles_bin_above_twice_the_error(O, sf, hann):
    """Detector alone (rate 0), then behind the estimate of a bin-0 sync pair: wherever the
    float64 margin exceeds 2 n1 (e_ref + E) the float64 argmax is the oracle's symbol."""
    N = 1 << sf
    E = (8.0 * sf + 42.0) * cc.U
    w = cc.hann_table(N) if hann else None
    decided = 0
    for y in cc.share_windows(sf, np.random.default_rng(90 + sf)):
        d, k = cc.margin_f64(y, 0.0, w)
        if d > 2.0 * E * np.abs(y.astype(np.complex128)).sum():
            decided += 1
            assert k == int(O.raw_demod(y, sf, 1, hann)[0])
    raw, deltas = cc.sweep_frames(O, sf, 1, 2)
    for f in range(2):
        row = O.dechirp(raw[f], sf, 1)
        syms, _, cfo, toff = O.lora_demodulate(row, sf, 1, hann)
        rate, t_off = cc.rate_of(cfo, sf), int(np.round(np.float32(toff)))
        for s, win in enumerate(cc.windows(O, row, sf, 1, "legacy", False, t_off)):
            if s < 2:
                continue
            d, k = cc.margin_f64(win, rate, w)
            wmax = np.uint32(cc.window_max(win)).view(np.float32)
            _, _, rmax, _, tabs = cc.bound_terms(sf, rate, rate, t_off)
            e_ref = cc.U * rmax * ((s + 1.0) * N + tabs + 2.0 * N)
            if d > 2.0 * (2.0 * N * float(wmax)) * (e_ref + E):
                decided += 1
                assert k == int(syms[s - 2]), (f, s, deltas[f, s - 2])
                if deltas[f, s - 2] != 0:  # the stronger tone: b for delta > 0, a for delta < 0
                    assert k == ((N // 2 + 9 + 7 * f) % N if deltas[f, s - 2] > 0 else (5 + 3 * f) % N)
    assert decided >= 40


@pytest.mark.parametrize("amp", [1.0, 0.4 / 1.7])
@pytest.mark.parametrize("variant", cc.VARIANTS, ids=cc.variant_id)
def test_each_sweep_holds_certified_and_rejected_symbols(O, variant, amp):
    """`certified` on the float64 margins of the sweep, with the oracle's offsets for both the
    exact and the speculative estimate (a bin-0 sync pair: no rotation either way)."""
    mode, sf, osr, window, dechirp = variant
    F = cc.frames_of(sf)
    w = cc.hann_table(1 << sf) if window == "hann" else None
    raw, deltas = cc.sweep_frames(O, sf, osr, F, amp, chirped_sync=mode != "api")
    x = cc.plan_input(O, raw, sf, osr, mode, dechirp)
    if mode == "legacy":
        peak = np.abs(np.ascontiguousarray(O.dechirp(raw[0], sf, osr)).view(np.float32)).max()
        assert (peak > 1.0) == (amp == 1.0)  # rescaled, or verbatim
    verdicts = []
    for f in range(F):
        _, _, cfo, toff = cc.oracle_frame(O, x[f], sf, osr, mode, dechirp, window == "hann")
        fp = {"rate": cc.rate_of(cfo, sf), "t_off": int(np.round(np.float32(toff)))}
        assert fp["t_off"] == 0 and abs(float(fp["rate"])) < 1e-6
        wins = cc.windows(O, x[f], sf, osr, mode, dechirp, fp["t_off"])
        for s in range(2, cc.S_TOTAL):
            d, _ = cc.margin_f64(wins[s][::osr], fp["rate"], w)
            wmax = np.uint32(cc.window_max(wins[s])).view(np.float32)
            ok = cc.certified(d, wmax, s, fp, fp, sf, mode)
            verdicts.append(ok)
            if abs(deltas[f, s - 2]) <= 2.0 ** -20:
                assert not ok, (f, s, deltas[f, s - 2], d)
    assert any(verdicts) and not all(verdicts), (sum(verdicts), len(verdicts))


@pytest.mark.parametrize("variant", [v for v in cc.VARIANTS if v[0] == "legacy" and not v[4]], ids=cc.variant_id)
def test_offsets_batch_holds_a_frame_whose_time_offsets_split(O, variant):
    mode, sf, osr, window, dechirp = variant
    hann = window == "hann"
    x, _ = cc.family_frames(O, variant, "offsets")
    pairs = [(cc.prepass_t_off(O, r, sf, osr, hann), cc.t_off_of(O.lora_demodulate(r, sf, osr, hann)[3])) for r in x]
    assert all(e != 0 for _, e in pairs), pairs  # t_off != 0 everywhere: e_ref's L term and moved windows
    assert [p != e for p, e in pairs] == [False] * (len(x) - 1) + [True], pairs
