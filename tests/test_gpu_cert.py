"""GPU: the certification of the speculative pipeline, per symbol.

tests/test_gpu_spec.py sees the pipeline through its final outputs, which the exact recompute
repairs whatever the symbol pass did.  Here ``DemodPlan.spec_trace()`` shows what the symbol
pass recorded and what the certification decided, and tests/cert_checker.py - a float64 model
checked against the CPU oracle in tests/test_cert_checker.py - holds both to account, for every
loop of the symbol pass (cert_checker.VARIANTS) and two input families: a sweep of near-ties
from "a tie in fp32" to "safely certified", rescaled and verbatim, and oracle-modulated frames
with a carrier offset and a delay, noiseless and at -10 dB.  Frames of 39 symbols, 5 or 3 per
batch, rows 3 samples apart.  Per case:

  1. symbols, sync, cfo and time_offset equal the oracle's, bit for bit;
  2. every data window's recorded maximum, and the frame's slot, are the model's bits;
  3. the reject list is exactly the set `certified` rejects on the GPU's own record, without
     duplicates, its length what the run added to spec_recomputed(); a frame whose two time
     offsets differ lists every data symbol and its sync pair;
  4. every recorded margin lies within 2 n1 (e_spec + E) of the float64 margin (a margin is the
     difference of two bins, each allowed n1 (e_spec + E)), and a certified symbol is the
     float64 argmax;
  5. every sweep symbol with |delta| <= 2^-20 is listed; no symbol whose float64 margin exceeds
     8 B is (the kernel needs 4 B, the margin may be off by item 4's amount).
"""
import ctypes as C

import numpy as np
import pytest

from tests import cert_checker as cc

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


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def reference(O):
    """The oracle's outputs per (mode, sf, osr, window, family), computed once: the fused and
    the plain variant of a configuration demodulate the same dechirped frames."""
    cache = {}

    def get(variant, family, x):
        mode, sf, osr, window, dechirp = variant
        key = (mode, sf, osr, window, family)
        if key not in cache:
            cache[key] = [cc.oracle_frame(O, x[f], sf, osr, mode, dechirp, window == "hann") for f in range(len(x))]
        return cache[key]

    return get


def run_plan(amd, variant, x):
    """`x` through a fresh plan of the variant, rows PAD samples apart with a large value
    between them (a read past a frame would show in the maxima): (plan, result, listed)."""
    mode, sf, osr, window, dechirp = variant
    F, L = x.shape
    big = np.full((F, L + cc.PAD), np.complex64(9.0 + 9.0j))
    big[:, :L] = x
    t = torch.from_numpy(big).cuda()[:, :L]
    assert t.stride(0) == L + cc.PAD
    plan = amd.DemodPlan(sf, osr, 125000, window, dechirp=dechirp, mode=mode)
    before = plan.spec_recomputed()
    res = plan.run(t)
    torch.cuda.synchronize()
    assert "spec" in plan.last_kernels()
    return plan, res, plan.spec_recomputed() - before


@pytest.mark.parametrize("family", cc.FAMILIES)
@pytest.mark.parametrize("variant", cc.VARIANTS, ids=cc.variant_id)
def test_certification_per_symbol(O, amd, reference, variant, family):
    mode, sf, osr, window, dechirp = variant
    x, deltas = cc.family_frames(O, variant, family)
    plan, res, added = run_plan(amd, variant, x)
    syms = res.symbols.cpu().numpy()
    sync, cfo, toff = res.sync.cpu().numpy(), res.cfo.cpu().numpy(), res.time_offset.cpu().numpy()
    # 1. the outputs
    for f, (osym, osync, ocfo, otoff) in enumerate(reference(variant, family, x)):
        np.testing.assert_array_equal(syms[f], osym, err_msg=f"frame {f} symbols")
        assert int(sync[f]) == osync, f"frame {f} sync"
        assert bits(cfo[f]) == bits(ocfo) and bits(toff[f]) == bits(otoff), f"frame {f} offsets"
    tr = plan.spec_trace()
    if mode != "raw":
        assert np.array_equal(bits(tr.fp["cfo"]), bits(cfo)) and np.array_equal(bits(tr.fp["time_offset"]), bits(toff))
    rep = cc.evaluate(O, variant, x, syms, tr, deltas)
    print(f"CERT_SLACK {cc.variant_id(variant)} {family}: worst |margin error| / (n1 (e_spec + E)) = "
          f"{rep['worst']:.4f}; listed {len(rep['listed'])}, t_off split in frames {rep['t_split']}")
    # 2. the maxima
    assert not rep["wmax_bad"], rep["wmax_bad"][:4]
    assert not rep["slot_bad"], rep["slot_bad"][:4]
    # 3. the decision
    assert len(set(rep["listed"])) == len(rep["listed"]), "duplicates on the reject list"
    assert set(rep["listed"]) == rep["expected"], (sorted(set(rep["listed"]) - rep["expected"])[:6],
                                                   sorted(rep["expected"] - set(rep["listed"]))[:6])
    assert len(rep["listed"]) == added
    if mode == "legacy" and family == "offsets":
        assert rep["t_split"], "no frame of the batch split its time offsets (cert_checker.offset_frames)"
    for f in rep["t_split"]:
        whole = {(f, s) for s in range(2, cc.S_TOTAL)} | {(f, cc.SYNC_PAIR)}
        assert whole <= set(rep["listed"]), f"frame {f}: time offsets differ, not every symbol listed"
    # 4. the accuracy
    assert not rep["over"], rep["over"][:4]
    assert not rep["argmax_bad"], rep["argmax_bad"][:4]
    # 5. soundness at the edge
    assert not rep["edge_missing"], rep["edge_missing"][:4]
    assert not rep["wide_listed"], rep["wide_listed"][:4]
    if family.startswith("sweep"):
        data = {(f, s) for f in range(x.shape[0]) for s in range(2, cc.S_TOTAL)}
        assert data & set(rep["listed"]) and data - set(rep["listed"])  # both outcomes occurred


def test_trace_refusals_that_need_a_plan(O, amd):
    """In the entry's order behind the argument checks of tests/test_cert_capi.py: a last call
    off the pipeline, then the symbol, workspace and list capacities."""
    from lora_phy_amd import _capi

    variant = ("legacy", 7, 1, "none", False)
    x, _ = cc.family_frames(O, variant, "sweep")
    F, L = x.shape
    t = torch.from_numpy(x).cuda()
    plan = amd.DemodPlan(7, 1, 125000, "none", pipeline="split")
    with pytest.raises(RuntimeError):
        plan.spec_trace()
    plan.run(t)
    with pytest.raises(_capi.LoraError) as e:
        plan.spec_trace()
    assert e.value.code == _capi.LORA_EINVAL and "did not take the speculative pipeline" in str(e.value)

    plan = amd.DemodPlan(7, 1, 125000, "none")
    plan.run(t)
    tr = plan.spec_trace()
    K = len(tr.rejected)
    assert K > 0
    _, _, ws, stream = plan._last_run
    total = L // 128
    fp = np.zeros((2, F), np.dtype(amd.demod.SPEC_FRAME_DTYPE))
    slot, ent, lst = np.zeros(F, np.uint32), np.zeros((F * total, 2), np.uint32), np.zeros((K, 2), np.uint32)

    def call(sym_cap=F * total, ws_bytes=ws.numel(), list_cap=K):
        o = _capi.SpecTraceOut(fp[0].ctypes.data, fp[1].ctypes.data, slot.ctypes.data, ent.ctypes.data, lst.ctypes.data,
                               F, sym_cap, list_cap)
        rc = plan._lib.lora_demod_spec_trace(plan._h, ws.data_ptr(), ws_bytes, F, L, C.byref(o), stream)
        return rc, plan._lib.lora_last_error().decode()

    need = plan._lib.lora_demod_workspace_bytes(plan._h, F, L)
    assert call(sym_cap=F * total - 1, ws_bytes=need - 1, list_cap=K - 1) == (_capi.LORA_ERANGE, "symbol capacity too small")
    assert call(ws_bytes=need - 1, list_cap=K - 1) == (_capi.LORA_ERANGE, "workspace too small")
    assert call(list_cap=K - 1) == (_capi.LORA_ERANGE, "list capacity too small")
    assert call()[0] == K
    assert np.array_equal(lst, tr.rejected) and np.array_equal(ent[:, 0].view(np.float32).reshape(F, total), tr.margin)
