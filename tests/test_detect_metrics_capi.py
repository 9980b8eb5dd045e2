"""CPU: the detector-metrics entry point (lora_demod_metrics_batch) is declared, exported and
bound, rejects a NULL plan before any HIP call, and the host checker the GPU tests compare
against (tests/detect_checker.py) is itself pinned: to the reference's compiled
LoRaDetector<float>::detect by tests/golden/detect_metrics.json, bit for bit, and to the
oracle's symbols and sync words over the STRESS cases (the window construction).  The kernel
is checked by tests/test_gpu_detect_metrics.py on the GPU."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from lora_phy_amd import _capi
from tests import detect_checker as dc
from tests.golden_inputs import STRESS, dechirp, f32bits, sha, stress_input

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "lora_mi355x.h")
GOLD = os.path.join(REPO, "tests", "golden")
NAME = "lora_demod_metrics_batch"


@pytest.fixture(scope="module")
def O():
    from oracle.pyoracle import Oracle

    return Oracle()


def test_header_declares_library_exports_and_binding_is_set():
    text = open(HEADER).read()
    bare = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert NAME in re.findall(r"^[A-Za-z_][\w\s\*]*?\b(lora_\w+)\s*\(", bare, flags=re.M)
    assert NAME in _capi.EXPORTED_SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert NAME in {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    fn = getattr(_capi.lib(), NAME)
    assert fn.restype is C.c_int64
    assert fn.argtypes is not None and len(fn.argtypes) == 10
    # the header comment cites the reference lines, like its neighbours
    i = text.index(NAME + "(")
    assert re.search(r"\.(cpp|hpp):\d+", text[text.rindex("/*", 0, i):i])


def test_struct_mirror_lists_the_header_fields_in_order():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\}\s*lora_symbol_metrics;", text).group(1)
    assert re.findall(r"(\w+)\s*;", body) == [f for f, _ in _capi.SymbolMetrics._fields_]
    assert C.sizeof(_capi.SymbolMetrics) == 4 * C.sizeof(C.c_void_p) + 8


def test_null_plan_is_rejected_with_a_message():
    lib = _capi.lib()
    m = _capi.SymbolMetrics(None, None, None, None, 0)
    assert lib.lora_demod_metrics_batch(None, None, 0, 0, 0, None, None, None, C.byref(m), None) == _capi.LORA_EINVAL
    assert lib.lora_last_error().decode()
    assert lib.lora_demod_metrics_batch(None, None, 1, 128, 128, None, None, None, None, None) == _capi.LORA_EINVAL


def test_detect_metrics_has_no_cpu_fallback():
    import torch

    import lora_phy_amd as amd

    assert amd.DetectMetrics is amd.demod.DetectMetrics
    plan = object.__new__(amd.DemodPlan)  # no GPU is needed to reach the argument check
    plan.device, plan.mode, plan.step = torch.device("cuda", 0), "raw", 128
    with pytest.raises(TypeError):
        amd.DemodPlan.detect_metrics(plan, torch.zeros(256, dtype=torch.complex64))
    plan._h = None  # (close() in __del__ finds nothing to destroy)


def test_snr_helpers_are_plain_tensor_ops():
    import torch

    import lora_phy_amd as amd

    inf = float("inf")
    p = torch.tensor([[0.0, -1.0, -3.0, -0.5], [0.0, 0.0, -2.0, -inf]])
    a = torch.tensor([[-20.0, -inf, -13.0, -10.25], [-5.0, -6.0, -inf, -inf]])
    m = amd.DetectMetrics(p, a, torch.zeros_like(p), torch.zeros(2, 4, dtype=torch.uint16))
    snr = m.snr_db.numpy()
    assert np.array_equal(snr[0], np.float32([20.0, inf, 10.0, 9.75]))
    assert snr[1, 2] == inf and np.isnan(snr[1, 3])
    assert m.frame_snr_db().numpy()[0] == np.float32((10.0 + 9.75) / 2)
    assert m.frame_snr_db(first=0).numpy()[0] == inf


def test_checker_reproduces_the_reference_records(O):
    """Every record of detect_metrics.json (the reference's compiled detect()): the window is
    regenerated and sha-checked, then index and the three floats' bits must be equal."""
    with open(os.path.join(GOLD, "detect_metrics.json")) as fh:
        recs = json.load(fh)["records"]
    assert {r["sf"] for r in recs} == set(dc.GOLDEN_SFS)
    seen = 0
    for sf in dc.GOLDEN_SFS:
        wins = dc.golden_windows(O, sf)
        mine = [r for r in recs if r["sf"] == sf]
        assert [r["name"] for r in mine] == [n for n, _ in wins]
        for r, (name, w) in zip(mine, wins):
            assert sha(w) == r["sha256"], f"SF{sf} {name}: input generator drifted; regenerate the fixture"
            idx, p, pav, fi = dc.detect(O.fft(w))
            got = (idx, f32bits(p), f32bits(pav), f32bits(fi))
            assert got == (r["index"], r["power"], r["power_avg"], r["f_index"]), (sf, name)
            seen += 1
    assert seen == len(recs) >= 7 * 12


def test_reference_edge_rows():
    """The consequences the fixture must show (all-zero, constant, alternating windows)."""
    with open(os.path.join(GOLD, "detect_metrics.json")) as fh:
        recs = json.load(fh)["records"]
    ninf = f32bits(-np.inf)
    for r in recs:
        N = 1 << r["sf"]
        if r["name"] == "zero":
            assert (r["index"], r["power"], r["power_avg"], r["f_index"]) == (0, ninf, ninf, 0)
        elif r["name"] == "constant":
            # the peak is N: 20 log10f(N) against float(20 log10(N)) is 0 exactly where the two
            # round alike (SF 6, 7, 10, 12 in the reference's build), else a few ulp of 20 log10 N
            assert (r["index"], r["power_avg"], r["f_index"]) == (0, ninf, 0)
            assert abs(float(np.uint32(r["power"]).view(np.float32))) < 1e-5
            if r["sf"] in (6, 7, 10, 12):
                assert r["power"] == 0
        elif r["name"] == "alternating":
            assert (r["index"], r["power_avg"], r["f_index"]) == (N // 2, ninf, 0)
            assert abs(float(np.uint32(r["power"]).view(np.float32)) + 6.0206) < 1e-4
        elif r["name"] == "clean_0":
            assert r["index"] == 0
        elif r["name"] == "clean_last":
            assert r["index"] == N - 1


def frame_max_amp(O, x, case):
    """LoRaDemod.cpp:59-67 over the (dechirped) frame."""
    sf, osr, _, dech = case[:4]
    y = dechirp(O, x, sf, osr) if dech else x
    if len(y) == 0:
        return np.float32(0)
    return np.float32(max(np.abs(y.real).max(), np.abs(y.imag).max()))


@pytest.mark.parametrize("ci", range(len(STRESS)))
def test_checker_windows_give_the_oracle_symbols(O, ci):
    """LEGACY window construction (SF 2-12, osr 1-4, both windows, dechirp on / off, both t_off
    signs, scaled / unscaled): the checker's index equals the oracle's symbols and sync nibbles."""
    case = STRESS[ci]
    sf, osr, hann, dech, F = case[:5]
    with open(os.path.join(GOLD, "golden.json")) as fh:
        seed = json.load(fh)["stress"][ci]["seed"]
    x = stress_input(O, case, seed)
    syms, sync, cfo, toff, cnt = O.demod_frames(x, sf, osr, hann, dech)
    amp = np.array([frame_max_amp(O, x[f], case) for f in range(F)], np.float32)
    got = dc.frames_metrics(O, x, sf, osr, "legacy", hann, dech, 125000, cfo, toff, amp)
    total = x.shape[1] // ((1 << sf) * osr)
    assert got["index"].shape == (F, total)
    shift = max(sf - 4, 0)
    for f in range(F):
        if total >= 2:
            assert np.array_equal(got["index"][f, 2:], syms[f, :cnt[f]])
            nib = ((int(got["index"][f, 0]) >> shift) & 15) << 4 | ((int(got["index"][f, 1]) >> shift) & 15)
            assert nib == int(sync[f])
        else:
            assert np.array_equal(got["index"][f], syms[f, :cnt[f]])
