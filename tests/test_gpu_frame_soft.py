"""GPU: the soft path through the self-describing frame - k_soft_bits_frame behind
lora_demod_soft_bits_frame_batch and DemodPlan.soft_bits(reduced=), k_frame_decode_soft behind
lora_decode_frame_soft_batch and codec.decode_header_soft / decode_frame_soft - against the host
checker (tests/frame_soft_checker.py, itself checked on the CPU by
tests/test_frame_soft_checker.py).  Every float is compared by its bit pattern, everything
decoded as integers."""
import numpy as np
import pytest

from tests import detect_checker as dc
from tests import frame_checker as fc
from tests import frame_soft_checker as fs
from tests.test_soft_checker import NOISY_DB

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SFS = range(7, 13)


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


def assert_llr_bits(got, want, what=""):
    g, w = dc.bits(got), dc.bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.argwhere(g != w)
    assert len(bad) == 0, (what, len(bad), bad[:4].tolist(), [(got[tuple(b)], want[tuple(b)]) for b in bad[:4]])


# ---- reduced soft bits -------------------------------------------------------------------------
def raw_frames(O, sf):
    """Three frames of 12 symbols for a raw dechirping plan: a noiseless one whose columns 2 - 9
    are tones at bins N-2, N-1, 0, 1, 2, 4g-1, 4g+1, 4g+2 (the rotation's wrap and both sides of
    the rounding boundary), and two noisy ones."""
    N = 1 << sf
    g = 5
    rng = np.random.default_rng(700 + sf)
    edge = [N - 2, N - 1, 0, 1, 2, 4 * g - 1, 4 * g + 1, 4 * g + 2, 3, N // 2 + 1]
    rows = [O.lora_modulate(np.array(edge, np.uint16), sf, 1, 125000, 1.0, 0x12)]
    sigma = 10.0 ** (-NOISY_DB.get(sf, -8.0 - 3.0 * (sf - 7)) / 20.0)
    for _ in range(2):
        x = O.lora_modulate(rng.integers(0, N, 10).astype(np.uint16), sf, 1, 125000, 1.0, 0x12)
        rows.append(x + sigma * (rng.standard_normal(len(x)) + 1j * rng.standard_normal(len(x))))
    return np.stack(rows).astype(np.complex64)


def spectra(O, x, sf):
    return [[O.fft(w) for w in dc.frame_windows(O, row, sf, 1, "raw", False, True)] for row in x]


@pytest.mark.parametrize("sf", SFS)
def test_reduced_soft_bits_equal_the_checker(O, amd, sf):
    """Each SF is a template instance of its own (the cross-lane depth changes at SF 10, the
    reduction over waves starts at SF 11)."""
    x = raw_frames(O, sf)
    X = spectra(O, x, sf)
    plan = amd.DemodPlan(sf, dechirp=True, mode="raw")
    xt = torch.from_numpy(x).cuda()
    plain = plan.soft_bits(xt).cpu().numpy()
    for red in ((2, 8), (0, 12), (0, 0)):
        got = plan.soft_bits(xt, reduced=red).cpu().numpy()
        assert got.shape == (3, 12, sf) and got.dtype == np.float32
        want = np.stack([fs.soft_bits_frame(Xf, sf, red) for Xf in X])
        assert_llr_bits(got, want, (sf, red))
        assert not np.isnan(got).any()
        if red == (0, 0):
            assert_llr_bits(got, plain, (sf, "red_count 0 is the plain entry"))
    # the noiseless tones: every reduced LLR is decided, and for the value the hard rounding gives
    got = plan.soft_bits(xt, reduced=(2, 8)).cpu().numpy()[0, 2:10, :sf - 2]
    N = 1 << sf
    bins = np.array([N - 2, N - 1, 0, 1, 2, 19, 21, 22])
    v = fs.reduced_value(bins, sf)
    assert (got != 0).all() and np.array_equal(got > 0, ((v[:, None] >> np.arange(sf - 2)[None, :]) & 1) == 1)


def test_sf7_workgroup_boundary_inside_the_reduced_columns(O, amd):
    """33 frames of 12 symbols at SF 7 (G = 32 symbols per workgroup): groups end at work items
    32, 64, ... - column 8 of frame 2, column 4 of frame 5, ... - inside the reduced columns.
    The 33 are drawn from three, which keeps the checker to three frames."""
    sf = 7
    base = raw_frames(O, sf)
    pick = np.arange(33) % 3
    want3 = np.stack([fs.soft_bits_frame(Xf, sf, (2, 8)) for Xf in spectra(O, base, sf)])
    plan = amd.DemodPlan(sf, dechirp=True, mode="raw")
    out = torch.full((35, 14, sf), -7.5, device="cuda")
    view = plan.soft_bits(torch.from_numpy(base[pick]).cuda(), reduced=(2, 8), out=out)
    assert view.shape == (33, 12, sf)
    o = out.cpu().numpy()
    assert_llr_bits(o[:33, :12], want3[pick], "33 frames")
    assert (o[33:] == -7.5).all() and (o[:, 12:] == -7.5).all()


def test_legacy_frames_with_offsets(O, amd):
    """A legacy plan (the stream receiver's): the windows follow the frame's cfo, time offset and
    maximum amplitude, and columns 2 - 9 are reduced."""
    sf = 8
    rng = np.random.default_rng(8)
    rows = []
    for n in (3, 9):
        sym = fc.encode_frame(rng.integers(0, 256, n).astype(np.uint8).tobytes(), sf, 1, 1)[:18]
        x = O.lora_modulate(sym, sf, 1, 125000, 1.0, 0x12)
        rows.append(x + 0.2 * (rng.standard_normal(len(x)) + 1j * rng.standard_normal(len(x))))
    x = np.stack(rows).astype(np.complex64)
    plan = amd.DemodPlan(sf, dechirp=True)
    xt = torch.from_numpy(x).cuda()
    res = plan.run(xt)
    got = plan.soft_bits(xt, res, reduced=(2, 8)).cpu().numpy()
    want = fs.soft_bits_frames(O, x, sf, 1, "legacy", False, True, 125000, res.cfo.cpu().numpy(),
                               res.time_offset.cpu().numpy(), res.max_amp.cpu().numpy(), (2, 8))
    assert_llr_bits(got, want, "legacy")
    assert np.array_equal(res.max_amp.cpu().numpy(), [fs.max_amplitude(O, r, sf) for r in x])


def test_capi_rules_with_a_plan(amd):
    from lora_phy_amd import _capi

    lib = _capi.lib()
    N, F, total, sf = 128, 2, 12, 7
    L = total * N
    iq = torch.zeros((F, L), dtype=torch.complex64, device="cuda")
    buf = torch.full((F, total, sf), 3.0, device="cuda")
    raw, sf6 = amd.DemodPlan(7, mode="raw"), amd.DemodPlan(6, mode="raw")

    def call(plan, first, count, frames=F, frame_len=L, lstride=total, llr=buf):
        return lib.lora_demod_soft_bits_frame_batch(plan._h, iq.data_ptr(), frames, frame_len, frame_len, None, None,
                                                    None, llr.data_ptr() if llr is not None else None, lstride,
                                                    first, count, None)

    E = _capi.LORA_EINVAL
    for first, count in ((-1, 2), (2, -1), (5, 8), (13, 0), (0, 13), (1 << 62, 1 << 62)):
        assert call(raw, first, count) == E and lib.lora_last_error().decode(), (first, count)
    assert call(sf6, 2, 8, frame_len=12 * 64) == E                # SF 6 has no header block
    assert call(raw, 2, 8, lstride=total - 1) == E and call(raw, 2, 8, frames=-1) == E
    torch.cuda.synchronize()
    assert (buf == 3.0).all()  # nothing ran
    assert call(raw, 2, 8, frames=0) == total and call(raw, 2, 8, llr=None, lstride=0) == total
    assert call(sf6, 12, 0, frame_len=12 * 64, llr=None, lstride=0) == total  # red_count 0: the plain entry's rules
    torch.cuda.synchronize()
    assert (buf == 3.0).all()
    assert call(raw, 4, 8) == total  # the row's last columns
    torch.cuda.synchronize()
    assert (dc.bits(buf.cpu().numpy()) == 0).all()  # zero frames: every LLR +0.0
    with pytest.raises(_capi.LoraError):
        raw.soft_bits(iq, reduced=(6, 8))
    with pytest.raises(_capi.LoraError):
        sf6.soft_bits(torch.zeros((1, 12 * 64), dtype=torch.complex64, device="cuda"), reduced=(2, 8))


# ---- decode_frame_soft and decode_header_soft --------------------------------------------------
def sizes(sf):
    return (0, 1, 2, 3, 4, 5, sf, 16, 17, 255)


def batch_of(cases, sf, seed):
    """[F, S, sf] LLRs of frames of different lengths: each row's own, then seeded noise."""
    S = max(len(c) for c in cases)
    a = np.random.default_rng(seed).standard_normal((len(cases), S, sf)).astype(np.float32)
    for f, c in enumerate(cases):
        a[f, :len(c)] = c
    return a


def same_decode(amd, a, sf, avail=None, max_bytes=None, max_flips=5, what=""):
    """codec.decode_frame_soft (max_bytes None: decode_header_soft) against the checker."""
    t = torch.from_numpy(a).cuda()
    av = None if avail is None else torch.from_numpy(np.asarray(avail, np.int32)).cuda()
    if max_bytes is None:
        got = amd.codec.decode_header_soft(t, sf, av, max_flips)
        assert got.payload is None
    else:
        got = amd.codec.decode_frame_soft(t, sf, av, max_bytes, max_flips)
    torch.cuda.synchronize()
    want = fs.decode_batch(a, sf, avail, max_bytes, max_flips)
    for name, key in (("status", "status"), ("nbytes", "nbytes"), ("rdd", "rdd"), ("has_crc", "crc"),
                      ("nsym", "nsym"), ("errors", "errors"), ("hdr_flips", "hdr_flips")):
        g = getattr(got, name).cpu().numpy()
        assert g.dtype == np.int32 and np.array_equal(g, want[key]), (what, name, g.tolist(), want[key].tolist())
    if max_bytes is not None:
        assert np.array_equal(got.payload.cpu().numpy(), want["payload"]), what
    return want


@pytest.fixture(scope="module")
def grid():
    """Per SF the 100 frames of the grid (rdd 0-4 x crc x ten sizes) as clean LLRs of seeded
    magnitudes, with the planted (n, rdd, crc, payload)."""
    out = {}
    for sf in SFS:
        cases, planted = [], []
        for rdd in range(5):
            for crc in (0, 1):
                for n in sizes(sf):
                    seed = 1000 * sf + 100 * rdd + 10 * crc + n
                    pay = np.random.default_rng(seed).integers(0, 256, n).astype(np.uint8)
                    sym = fc.encode_frame(pay.tobytes(), sf, rdd, crc)
                    cases.append(fs.frame_llrs(sym, sf, np.random.default_rng(seed)))
                    planted.append((n, rdd, crc, pay))
        out[sf] = (cases, planted)
    return out


@pytest.mark.parametrize("sf", SFS)
def test_grid_decodes_as_the_checker_and_as_planted(amd, grid, sf):
    cases, planted = grid[sf]
    a = batch_of(cases, sf, sf)
    nsym = np.array([len(c) for c in cases], np.int32)
    want = same_decode(amd, a, sf, nsym, 255, what=("grid", sf))
    assert (want["status"] == fc.OK).all() and not want["errors"].any() and not want["hdr_flips"].any()
    for f, (n, rdd, crc, pay) in enumerate(planted):
        assert (want["nbytes"][f], want["rdd"][f], want["crc"][f]) == (n, rdd, crc)
        assert np.array_equal(want["payload"][f, :n], pay)
    same_decode(amd, a, sf, nsym, None, what=("grid headers", sf))


def damaged(cases, sf, seed):
    """The grid's short frames, hurt: two weak wrong bits in one header codeword; sign flips
    sprinkled over the whole frame (weak and full); zeros, +-inf and NaN among the LLRs; exact
    ties."""
    rng = np.random.default_rng(seed)
    out = []
    for c in cases:
        if len(c) > 60:
            continue
        kind = len(out) % 4
        llr = c.copy()
        if kind == 0:
            j = int(rng.integers(0, 5))
            for bit in rng.choice(8, 2, replace=False):
                r, col = fs.header_cell(sf, j, int(bit))
                llr[r, col] = -np.sign(llr[r, col]) * np.float32(rng.uniform(0.1, 0.4))
        elif kind == 1:
            hit = rng.random(llr.shape) < 0.06
            llr[hit] *= np.float32(-0.3)
            hit = rng.random(llr.shape) < 0.02
            llr[hit] *= np.float32(-1.0)
        elif kind == 2:
            flat = llr.reshape(-1)
            for val in (0.0, -0.0, np.inf, -np.inf, np.nan):
                flat[rng.integers(0, flat.size, max(1, flat.size // 40))] = np.float32(val)
        else:
            flip = np.where(rng.random(llr.shape) < 0.05, np.float32(-1.0), np.float32(1.0))
            llr[:, :] = flip * np.sign(llr) * np.abs(llr).round()  # magnitudes 0, 1 and 2: exact ties
        out.append(llr)
    return out


@pytest.mark.parametrize("sf", SFS)
def test_damaged_frames_every_group_size_avail_and_max_flips(amd, grid, sf):
    cases = damaged(grid[sf][0], sf, 50 + sf)
    assert len(cases) >= 40
    a = batch_of(cases, sf, 100 + sf)
    nsym = np.array([len(c) for c in cases], np.int32)
    seen = set()
    # max_bytes 0, 2, 6, 14, 30 and 62: groups of 2, 4, 8, 16, 32 and 64 lanes; header-only mode: 1
    for max_bytes, max_flips in ((None, 5), (0, 5), (2, 40), (6, 0), (14, 5), (30, 40), (62, 5), (255, 0)):
        want = same_decode(amd, a, sf, nsym, max_bytes, max_flips, (sf, max_bytes, max_flips))
        seen |= set(want["status"].tolist())
        if max_flips == 40:
            assert want["hdr_flips"].max() >= 2
    assert seen == {fc.OK, fc.HEADER, fc.SHORT, fc.CRC}
    # avail from 0 to beyond the frame, and none given (the whole row, noise included)
    rng = np.random.default_rng(sf)
    avail = nsym + rng.integers(-3, 4, len(nsym)).astype(np.int32)
    avail[:6] = [0, 7, 8, -5, a.shape[1], a.shape[1] + 9]
    same_decode(amd, a, sf, avail, 30, 5, (sf, "avail"))
    same_decode(amd, a, sf, avail, None, 5, (sf, "avail, header"))
    same_decode(amd, a, sf, None, 30, 40, (sf, "no avail"))


def test_views_single_frames_outputs_given_and_refusals(amd, grid):
    sf = 9
    cases = damaged(grid[sf][0], sf, 3)[:37]
    a = batch_of(cases, sf, 4)
    wide = np.random.default_rng(5).standard_normal((a.shape[0], a.shape[1] + 5, sf)).astype(np.float32)
    wide[:, 2:2 + a.shape[1]] = a
    t = torch.from_numpy(wide).cuda()
    view = t[:, 2:2 + a.shape[1]]  # columns 2 onward of a wider tensor, as the chain passes them
    want = fs.decode_batch(a, sf, None, 20, 5)
    got = amd.codec.decode_frame_soft(view, sf, max_bytes=20)
    assert np.array_equal(got.status.cpu().numpy(), want["status"])
    assert np.array_equal(got.payload.cpu().numpy(), want["payload"])
    # outputs given: written in place, nothing beyond the payload's width
    pay = torch.full((len(cases), 24), 7, dtype=torch.uint8, device="cuda")
    out = amd.codec.FrameResult(*(torch.full((len(cases),), -9, dtype=torch.int32, device="cuda") for _ in range(6)),
                                payload=pay[:, :20],
                                hdr_flips=torch.full((len(cases),), -9, dtype=torch.int32, device="cuda"))
    assert amd.codec.decode_frame_soft(view, sf, max_bytes=20, out=out) is out
    assert np.array_equal(out.hdr_flips.cpu().numpy(), want["hdr_flips"])
    assert np.array_equal(out.payload.cpu().numpy(), want["payload"])
    assert (pay.cpu().numpy()[:, 20:] == 7).all()
    one = amd.codec.decode_frame_soft(torch.from_numpy(a[3]).cuda(), sf, max_bytes=20)
    assert one.payload.shape == (20,) and np.array_equal(one.payload.cpu().numpy(), want["payload"][3])
    none = amd.codec.decode_frame_soft(torch.zeros((0, 12, sf), device="cuda"), sf)
    assert none.status.shape == (0,) and none.payload.shape[0] == 0
    with pytest.raises(TypeError):
        amd.codec.decode_frame_soft(t.double(), sf)
    with pytest.raises(ValueError):
        amd.codec.decode_frame_soft(t, sf + 1)
    with pytest.raises(ValueError):
        amd.codec.decode_frame_soft(t, sf, max_flips=41)
    with pytest.raises(ValueError):
        amd.codec.decode_header_soft(t, sf, max_flips=-1)
    with pytest.raises(ValueError):
        amd.codec.decode_frame_soft(t, sf, max_bytes=256)
    with pytest.raises(amd._capi.LoraError):
        amd.codec.decode_frame_soft(torch.zeros((1, 12, 6), device="cuda"), 6)


def test_soft_bits_into_the_frame_decoder(O, amd):
    """Modulated frames in noise -> run -> soft_bits(reduced=(2, 8)) -> decode_frame_soft, against
    the checker on the oracle's windows, and against the hard decode of the same run."""
    sf, n, F = 7, 14, 24
    rng = np.random.default_rng(21)
    pays = rng.integers(0, 256, (F, n)).astype(np.uint8)
    rows = []
    for p in pays:
        x = O.lora_modulate(fc.encode_frame(p.tobytes(), sf, 1, 1), sf, 1, 125000, 1.0, 0x12)
        rows.append(x + 10.0 ** (6.5 / 20.0) * (rng.standard_normal(len(x)) + 1j * rng.standard_normal(len(x))))
    x = np.stack(rows).astype(np.complex64)
    plan = amd.DemodPlan(sf, dechirp=True)
    xt = torch.from_numpy(x).cuda()
    res = plan.run(xt)
    llr = plan.soft_bits(xt, res, reduced=(2, 8))
    soft = amd.codec.decode_frame_soft(llr[:, 2:], sf, max_bytes=n)
    hard = amd.codec.decode_frame(res.symbols, sf, max_bytes=n)
    torch.cuda.synchronize()
    want_llr = fs.soft_bits_frames(O, x, sf, 1, "legacy", False, True, 125000, res.cfo.cpu().numpy(),
                                   res.time_offset.cpu().numpy(), res.max_amp.cpu().numpy(), (2, 8))
    assert_llr_bits(llr.cpu().numpy(), want_llr, "chain")
    want = fs.decode_batch(want_llr[:, 2:], sf, None, n, 5)
    for name, key in (("status", "status"), ("nbytes", "nbytes"), ("errors", "errors"), ("hdr_flips", "hdr_flips")):
        assert np.array_equal(getattr(soft, name).cpu().numpy(), want[key]), name
    assert np.array_equal(soft.payload.cpu().numpy(), want["payload"])
    ok_soft = (soft.status.cpu().numpy() == fc.OK) & (soft.payload.cpu().numpy() == pays).all(1)
    ok_hard = (hard.status.cpu().numpy() == fc.OK) & (hard.payload.cpu().numpy() == pays).all(1)
    print(f"frames right of {F}: hard {int(ok_hard.sum())}, soft {int(ok_soft.sum())}")
    assert ok_soft.sum() >= ok_hard.sum()
    assert hard.hdr_flips is None
