"""CPU: the raw sample conversion's host model (tests/raw_checker.py, to_cf32) against the
header's formula evaluated in float64 and rounded once, over every code of every format; and the
Python layer's own statements of it (stream.raw_to_complex, stream.raw_scale, iq_io.quantize)
against the model, on CPU tensors."""
import numpy as np
import pytest

from tests import raw_checker as rk

torch = pytest.importorskip("torch")

DTYPES = [(np.int16, torch.int16), (np.int8, torch.int8), (np.uint8, torch.uint8)]
IDS = ["cs16", "cs8", "cu8"]


def all_codes(nd) -> np.ndarray:
    """Every code of the format as I, with Q running the other way: [codes, 2]."""
    info = np.iinfo(nd)
    v = np.arange(info.min, info.max + 1, dtype=np.int64)
    return np.stack([v, v[::-1]], axis=-1).astype(nd)


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("nd,td", DTYPES, ids=IDS)
def test_to_cf32_is_the_formula_rounded_once(nd, td):
    """The conversion and the bias are exact, so ((double)v - bias) * (double)scale rounded to fp32
    is the definition: the product is the only rounding."""
    raw = all_codes(nd)
    assert len(raw) == (65536 if nd is np.int16 else 256)
    bias = 127.5 if nd is np.uint8 else 0.0
    for scale in (None, 3.0, 1e-3):
        s = rk.default_scale(nd) if scale is None else np.float32(scale)
        want = ((raw.astype(np.float64) - bias) * np.float64(s)).astype(np.float32)
        got = rk.to_cf32(raw, scale)
        assert got.dtype == np.complex64 and got.shape == (len(raw),)
        assert np.array_equal(bits(got.real), bits(want[:, 0]))
        assert np.array_equal(bits(got.imag), bits(want[:, 1]))


def test_default_scales():
    from lora_phy_amd import stream

    for (nd, td), want in zip(DTYPES, (1 / 32768, 1 / 128, 1 / 127.5)):
        assert stream.raw_scale(td) == float(np.float32(want)) == float(rk.default_scale(nd))
    with pytest.raises(TypeError):
        stream.raw_scale(torch.int32)


def test_cu8_midpoint_codes():
    for scale in (None, 2.0):
        s = rk.default_scale(np.uint8) if scale is None else np.float32(scale)
        got = rk.to_cf32(np.array([[127, 128]], np.uint8), scale)
        assert got[0].real == np.float32(-0.5) * s and got[0].imag == np.float32(0.5) * s
    # the signed formats have a true zero, and their extremes are -1 and just under 1
    assert rk.to_cf32(np.array([[0, -32768]], np.int16))[0] == complex(0.0, -1.0)
    assert rk.to_cf32(np.array([[127, -128]], np.int8))[0] == complex(127 / 128, -1.0)


@pytest.mark.parametrize("nd,td", DTYPES, ids=IDS)
def test_raw_to_complex_on_cpu_tensors_is_the_model(nd, td):
    from lora_phy_amd import stream

    raw = all_codes(nd)
    for scale in (None, 0.37, -1.0, float("inf")):
        got = stream.raw_to_complex(torch.from_numpy(raw), scale).numpy()
        want = rk.to_cf32(raw, scale)
        assert got.dtype == np.complex64 and got.shape == want.shape
        for g, w in ((got.real, want.real), (got.imag, want.imag)):
            nan = np.isnan(w)
            assert np.array_equal(np.isnan(g), nan) and np.array_equal(bits(g)[~nan], bits(w)[~nan])
    rows = stream.raw_to_complex(torch.from_numpy(raw).reshape(4, -1, 2))
    assert rows.shape == (4, len(raw) // 4)
    with pytest.raises(ValueError):
        stream.raw_to_complex(torch.zeros((5, 3), dtype=td))
    with pytest.raises(TypeError):
        stream.raw_to_complex(torch.zeros((5, 2), dtype=torch.int32))


@pytest.mark.parametrize("nd,td", DTYPES, ids=IDS)
def test_quantize_inverts_raw_to_complex_on_every_code(nd, td):
    from lora_phy_amd import iq_io, stream

    raw = torch.from_numpy(all_codes(nd))
    back = iq_io.quantize(stream.raw_to_complex(raw), td)
    assert back.dtype == td and back.shape == raw.shape and torch.equal(back, raw)
    back = iq_io.quantize(stream.raw_to_complex(raw, 0.25), td, 0.25)
    assert torch.equal(back, raw)


@pytest.mark.parametrize("fmt", ["cs16", "cu8"])
@pytest.mark.parametrize("kind", ["integer", "rational"])
def test_the_host_model_recovers_the_planted_frames_from_the_quantised_capture(kind, fmt):
    """What tests/test_gpu_raw_samples.py's end-to-end cases rely on: to_cf32, the bank's host
    model, the host scan and finder and the oracle's demodulator on the cut frames return every
    planted frame's channel, start and symbols from the quantised capture."""
    from oracle.pyoracle import Oracle
    from tests import channel_checker as cc
    from tests import resample_checker as rc
    from tests import scan_checker as sc
    from tests.test_gpu_raw_samples import E2E, e2e_case

    O = Oracle()
    sf, osr, Li, D, period, T, cutoff, rows, steps = E2E[kind]
    raw, taps, channel, starts, syms = e2e_case(kind, fmt)
    x = rk.to_cf32(raw)
    rows_out = (cc.channelize_host(x, taps, steps, period, D) if Li == 1 else
                rc.resample_host(x, taps, steps, period, Li, D))
    step = (1 << sf) * osr
    hop, S = step // 4, syms.shape[1]
    frame_len = (S + 2) * step
    for c in range(len(steps)):
        y = rows_out[c]
        found = sc.find_frames_host(sc.scan_host(O, y, sf, osr, hop, dechirp=True), hop, sf, osr, S, 0x12,
                                    row_len=len(y))
        want = starts[channel == c]
        assert found.shape == want.shape and (np.abs(found - want) <= osr).all(), (c, found, want)
        cut = np.stack([y[s:s + frame_len] for s in found])
        o_syms, o_sync, _, _, cnt = O.demod_frames(cut, sf, osr, False, True)
        assert (np.asarray(cnt) == S).all()
        assert np.array_equal(np.asarray(o_syms)[:, :S] % (1 << sf), syms[channel == c]), c
        assert (np.asarray(o_sync) == 0x12).all(), c


@pytest.mark.parametrize("nd,td", DTYPES, ids=IDS)
def test_quantize_clamps_and_rounds_to_even(nd, td):
    from lora_phy_amd import iq_io

    info = np.iinfo(nd)
    x = torch.tensor([complex(1e9, -1e9), complex(float("inf"), float("-inf")), complex(1.0, -1.0)],
                     dtype=torch.complex64)
    got = iq_io.quantize(x, td).numpy()
    assert got[:2].tolist() == [[info.max, info.min]] * 2
    # +1.0 is one code past the top of the signed formats and cu8's top; -1.0 is every format's
    # lowest code
    assert got[2].tolist() == [info.max, info.min]
    # ties go to even: with scale 1 and no bias, 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, -0.5 -> 0, -1.5 -> -2
    if nd is not np.uint8:
        t = torch.tensor([complex(0.5, 1.5), complex(2.5, -0.5), complex(-1.5, -2.5)], dtype=torch.complex64)
        assert iq_io.quantize(t, td, 1.0).numpy().tolist() == [[0, 2], [2, 0], [-2, -2]]
    else:  # bias 127.5: x = 0 is the tie between 127 and 128, x = 1 between 128 and 129
        t = torch.tensor([complex(0.0, 1.0), complex(-1.0, 2.0)], dtype=torch.complex64)
        assert iq_io.quantize(t, td, 1.0).numpy().tolist() == [[128, 128], [126, 130]]
    with pytest.raises(TypeError):
        iq_io.quantize(x, torch.int32)
    with pytest.raises(TypeError):
        iq_io.quantize(x.real, td)
