"""GPU: the propagation stage (lora_phy_amd.stream.propagate, lora_propagate_batch) against the
numpy restatement of its definition (tests/propagate_checker.py): every comparison is ``==`` on
the bits.  The shapes are the smallest at which the kernel can go wrong: a workgroup owns 1024
slots of a row on the 16-byte grid of ``out`` and a lane two pairs of them, a path's samples are
staged on the 16-byte grid of ``in``, so the lengths sit round one tile and two, the views start on
even and odd samples, strides are even and odd, and the windows leave taps hanging over both ends
of ``in``."""
import numpy as np
import pytest

from tests import impair_checker as ic
from tests import propagate_checker as pc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
W = pc.delay_word


@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import lora_phy_amd

    return lora_phy_amd


def bits(a):
    return np.ascontiguousarray(a, np.complex64).view(np.uint32)


def samples(rows, L, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((rows, L)) + 1j * rng.standard_normal((rows, L))).astype(np.complex64)


def words(v, R, P=None):
    """The checker's integer words as the device tensor the C entry takes: [R] or [R, P] int64."""
    a = np.array(np.broadcast_to(np.asarray(v, dtype=object), (R,) if P is None else (R, P)).tolist(), np.int64)
    return torch.from_numpy(a).cuda()


def dev_params(kw, R):
    """The checker's keyword arguments as ``propagate``'s, everything as the device arrays of the C
    entry: int64 words, complex gains, an int32 phase."""
    d = np.asarray(kw.get("delay", 0), dtype=object)
    g = np.asarray(kw.get("gain", 1.0), np.complex64)
    P = max(d.shape[-1] if d.ndim else 1, g.shape[-1] if g.ndim else 1)
    out = dict(delay=words(d, R, P), gain=torch.from_numpy(np.array(np.broadcast_to(g, (R, P)))).cuda())
    for k, name in (("sfo", "sfo_ppm"), ("fcw", "cfo"), ("rate", "drift")):
        if kw.get(k) is not None:
            out[name] = words(kw[k], R)
    if kw.get("phase") is not None:
        ph = np.array(np.broadcast_to(np.asarray(kw["phase"], np.int64), (R,)))
        out["phase"] = torch.from_numpy(ph.astype(np.int32)).cuda()
    if kw.get("table") is not None:
        out["table"] = torch.from_numpy(np.ascontiguousarray(kw["table"], np.float32)).cuda()
    for k in ("in_first", "first_sample"):
        if k in kw:
            out[k] = kw[k]
    return out


def run(amd, x, length, in_off=0, out_off=0, pad=3, **kw):
    """``propagate`` on views of larger buffers: row r of the input begins ``in_off + r * (L + pad)``
    samples into its buffer, of the output ``out_off + r * (length + pad + 2)`` samples into its
    own, which is filled with a sentinel first; everything outside the rows must still hold it.
    Returns the result as numpy complex64 [R, length]."""
    R, L = x.shape
    si, so = L + pad, length + pad + 2
    buf = torch.zeros(in_off + R * si + 1, dtype=torch.complex64, device="cuda")
    xin = buf[in_off:in_off + R * si].view(R, si)[:, :L]
    xin.copy_(torch.from_numpy(x).cuda())
    obuf = torch.full((out_off + R * so + 1,), SENTINEL, dtype=torch.complex64, device="cuda")
    before = obuf.clone()

    def rows_of(b):
        return b[out_off:out_off + R * so].view(R, so)[:, :length]

    out = rows_of(obuf)
    got = amd.stream.propagate(xin, length=length, out=out, **dev_params(kw, R))
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and got.shape == out.shape
    res = got.cpu().numpy().copy()
    out.copy_(rows_of(before))
    assert torch.equal(obuf.view(torch.uint8), before.view(torch.uint8)), "a sample outside the rows was written"
    return res


# three paths: delays of both signs, fractional and whole; three rows of their own clock and carrier
CHANNEL = dict(delay=[[W(2.3), W(-1.75), 5 << 32], [W(0.5), W(0.5), -(3 << 32)], [W(-7.996), 0, W(11.004)]],
               gain=[[1.0, 0.5j, -0.25 + 0.1j], [0.7 - 0.7j, 0.25, 1j], [1.0, -0.5, 0.125j]],
               sfo=[1 << 20, -(1 << 19), 85899], fcw=[123456789 << 32, -(7 << 40), 1 << 62],
               rate=[1 << 44, -(3 << 41), 118059162072], phase=[1 << 30, -5, -(1 << 31)])


@pytest.mark.parametrize("L", [1, 1023, 1024, 1025, 2500])
def test_lengths_rows_and_views(amd, L):
    """3 rows with padded strides, in and out views that start on an even and on an odd sample (so
    neither the 16-byte stores nor the staging are always aligned), in_len != row_len and in_first
    != first_sample, the window such that the taps hang over both ends of ``in``."""
    x = samples(3, L + 9, 100 + L)
    kw = dict(CHANNEL, first_sample=1000, in_first=1003)   # the window ends 6 samples after the outputs do
    want = pc.propagate_host(x, L, **kw)
    for in_off, out_off in ((0, 0), (1, 0), (0, 1), (1, 1)):
        got = run(amd, x, L, in_off, out_off, **kw)
        assert (bits(got) == bits(want)).all(), (L, in_off, out_off)
    # an even stride of in and an odd one of out put the rows at both alignments in one launch
    got = run(amd, x, L, 0, 0, pad=4, **kw)
    assert (bits(got) == bits(want)).all()
    one = run(amd, x[:1], L, 1, 1, **{k: (v[:1] if isinstance(v, list) else v) for k, v in kw.items()})
    assert (bits(one) == bits(want[:1])).all()


@pytest.mark.parametrize("T", [2, 16, 32])
@pytest.mark.parametrize("P", [1, 3, 8])
def test_taps_and_paths(amd, T, P):
    """Whole and fractional delays of both signs, two paths more than a tile apart, two with the
    same delay."""
    delays = [W(1500.3), W(-0.25), W(-0.25), 4 << 32, W(-1200.7), W(0.999), W(63.5), -(1 << 32)][:P]
    gains = [1.0, 0.5j, -0.5j, 0.25, -0.125 + 0.5j, 0.3, -0.2j, 0.1][:P]
    x = samples(2, 2400, 10 * T + P)
    kw = dict(delay=[delays], gain=[gains], sfo=[-(1 << 18), 1 << 17], table=pc.fracdelay_table(T),
              first_sample=77, in_first=100)
    want = pc.propagate_host(x, 2500, **kw)
    got = run(amd, x, 2500, 1, 0, **kw)
    assert (bits(got) == bits(want)).all()
    assert np.count_nonzero(want) > 500


@pytest.mark.parametrize("sign", [1, -1])
def test_clock_offset_steps_the_whole_sample(amd, sign):
    """sfo = +/-2^20 with delays whose fraction sits just under a whole sample, so that q steps
    inside a tile (output 300), at a tile's last slot and at the next tile's first (1023 | 1024 of
    an aligned ``out``, and one earlier for an ``out`` that starts on an odd sample)."""
    s = sign * (1 << 20)
    steps = [300, 1023, 1024, 1025]
    delay = [[-s * nc + sign, (2 << 32) - s * nc + sign] for nc in steps]
    x = samples(4, 2500, 5)
    kw = dict(delay=delay, gain=[[1.0, 0.5j]], sfo=s)
    n = np.arange(2500, dtype=np.int64)
    for r, nc in enumerate(steps):
        j0, _ = pc.positions(n, delay[r][0], s, 16)
        assert np.flatnonzero(np.diff(j0 - n)).tolist() == [nc - 1]   # q steps between outputs nc - 1 and nc
    want = pc.propagate_host(x, **kw)
    for out_off in (0, 1):
        got = run(amd, x, 2500, 0, out_off, **kw)
        assert (bits(got) == bits(want)).all(), out_off


@pytest.mark.parametrize("first", [(1 << 33) + 5, (1 << 40) - 1300])
def test_far_positions(amd, first):
    """first_sample = 2^33 + 5, and a row that ends at sample 2^40 exactly: the positions, the
    clock offset's product and the rotation's word are 64-bit."""
    L = 1300
    kw = dict(delay=[[W(0.37), W(-2.5)]], gain=[[1.0, -0.5j]], sfo=[1 << 20, -(1 << 20)],
              fcw=[(1 << 61) + 12345, -(5 << 40)], rate=[(3 << 30) + 1, -(1 << 25)], phase=[-9, 1 << 20])
    n = np.array([first, first + L - 1], np.int64)
    x = samples(2, L + 64, 6)
    # the clock offsets move the two rows' windows first / 2048 samples apart: a call for each, its
    # window beginning 3 samples after the first tap read
    for r in range(2):
        row = {k: [v[r]] if k in ("sfo", "fcw", "rate", "phase") else v for k, v in kw.items()}
        in_first = min(int(pc.positions(n, d, row["sfo"][0], 16)[0].min()) for d in kw["delay"][0]) + 3
        want = pc.propagate_host(x[r:r + 1], L, first_sample=first, in_first=in_first, **row)
        assert np.count_nonzero(want) > L // 2
        got = run(amd, x[r:r + 1], L, r, 1 - r, first_sample=first, in_first=in_first, **row)
        assert (bits(got) == bits(want)).all(), r


def test_splits_and_windows_equal_the_whole(amd):
    x = samples(3, 2509, 7)
    kw = dict(CHANNEL, first_sample=1000, in_first=1003)
    whole = run(amd, x, 2500, **kw)
    assert (bits(whole) == bits(pc.propagate_host(x, 2500, **kw))).all()
    for cut in (1, 1024, 1500):
        a = run(amd, x, cut, **kw)
        b = run(amd, x, 2500 - cut, 1, 1, **dict(kw, first_sample=1000 + cut))
        assert (bits(np.concatenate([a, b], axis=1)) == bits(whole)).all(), cut
    # outputs 1100 .. 1299 of the recording read samples 1100 - 12 - 8 - 1 .. 1299 + 8 + 8 + 1 at the most
    lo, hi = 1079 - 1003, 1317 - 1003
    part = run(amd, np.ascontiguousarray(x[:, lo:hi]), 200, 1, 0, **dict(kw, first_sample=1100, in_first=1003 + lo))
    assert (bits(part) == bits(whole[:, 100:300])).all()


@pytest.mark.parametrize("parts", [("fcw",), ("rate",), ("phase",), ("fcw", "rate"), ("fcw", "rate", "phase")])
def test_rotation_parts(amd, parts):
    x = samples(3, 1100, 8)
    kw = dict(delay=[[W(0.5)]], gain=[[1.0]], first_sample=(1 << 32) - 500, in_first=(1 << 32) - 500)
    kw.update({k: CHANNEL[k] for k in parts})
    got = run(amd, x, 1100, **kw)
    assert (bits(got) == bits(pc.propagate_host(x, **kw))).all()


def test_rotation_without_drift_is_impairs(amd):
    """rate absent and fcw = fcw32 << 32: the same rows through ``impair`` give the same bits."""
    x = torch.from_numpy(samples(3, 1500, 9)).cuda()
    fcw32 = np.array([123456789, -(1 << 31), 3], np.int64)
    ph = np.array([-77, 1 << 29, 0], np.int64)
    first = (1 << 33) + 5
    a = amd.stream.propagate(x, delay=0.0, cfo=torch.from_numpy(fcw32 << 32).cuda(),
                             phase=torch.from_numpy(ph.astype(np.int32)).cuda(), first_sample=first, in_first=first)
    b = amd.stream.impair(x, cfo=torch.from_numpy(fcw32.astype(np.int32)).cuda(),
                          phase=torch.from_numpy(ph.astype(np.int32)).cuda(), first_sample=first)
    torch.cuda.synchronize()
    assert (bits(a.cpu().numpy()) == bits(b.cpu().numpy())).all()
    want = ic.impair_host(x.cpu().numpy(), fcw=fcw32.tolist(), phase=ph.tolist(), first_sample=first)
    assert (bits(a.cpu().numpy()) == bits(want)).all()


def test_nan_and_inf_propagate(amd):
    """Non-finite samples spread over the taps as the arithmetic makes them: a NaN wherever the
    checker has one (sign and payload aside), the same bits everywhere else."""
    x = samples(2, 1200, 10)
    x[0, 100] = np.nan
    x[0, 500] = complex(np.inf, 1.0)
    x[1, 1023] = complex(2.0, -np.inf)
    x[1, 1199] = complex(np.nan, np.inf)
    for delay in ([[W(0.5), W(-3.25)]], [[0, 2 << 32]]):
        kw = dict(delay=delay, gain=[[1.0, 0.5j]], fcw=CHANNEL["fcw"][:2])
        want, got = pc.propagate_host(x, **kw), run(amd, x, 1200, **kw)
        for w, g in ((want.real, got.real), (want.imag, got.imag)):
            assert np.array_equal(np.isnan(w), np.isnan(g))
            ok = ~np.isnan(w)
            assert np.array_equal(w[ok].view(np.uint32), g[ok].view(np.uint32))
        assert np.isnan(want.real).sum() >= 4 and np.isfinite(want.real).sum() > 2000


def test_device_guard(amd):
    """The call leaves the current device unchanged, and on a second device, where there is one,
    computes what it computes on device 0."""
    torch.cuda.set_device(0)
    x = torch.from_numpy(samples(2, 1100, 11))
    outs = []
    for d in range(min(torch.cuda.device_count(), 2) - 1, -1, -1):
        y = amd.stream.propagate(x.to(f"cuda:{d}"), delay=[0.25, 1.5], gain=[1.0, 0.5j], sfo_ppm=20.0, cfo=0.01)
        assert torch.cuda.current_device() == 0
        torch.cuda.synchronize(d)
        assert y.device.index == d
        outs.append(y.cpu().numpy())
    want = pc.propagate_host(x.numpy(), delay=[[W(0.25), W(1.5)]], gain=[[1.0, 0.5j]], sfo=pc.sfo_word(20.0),
                             fcw=int(round(0.01 * 2.0 ** 64)))
    for got in outs:
        assert (bits(got) == bits(want)).all()


def test_python_forms(amd):
    """Scalars, per-row and per-path values, host values and device tensors: all reach the C entry
    as the same arrays."""
    x = samples(3, 1100, 12)
    xd = torch.from_numpy(x).cuda()
    get = lambda t: t.cpu().numpy()  # noqa: E731
    # everything scalar: one path
    got = get(amd.stream.propagate(xd, delay=0.25, gain=0.5 - 0.5j, sfo_ppm=-40.0, cfo=0.125, drift=1e-9, phase=0.25))
    want = pc.propagate_host(x, delay=W(0.25), gain=0.5 - 0.5j, sfo=pc.sfo_word(-40.0), fcw=1 << 61,
                             rate=int(round(1e-9 * 2.0 ** 64)), phase=1 << 30)
    assert (bits(got) == bits(want)).all()
    # per path, shared by the rows; an int is a word
    got = get(amd.stream.propagate(xd, delay=[0.0, 1.5, -2.75], gain=[1.0, 0.5j, -0.25], drift=118059162072))
    want = pc.propagate_host(x, delay=[[0, W(1.5), W(-2.75)]], gain=[[1.0, 0.5j, -0.25]], rate=118059162072)
    assert (bits(got) == bits(want)).all()
    # per row and path, per row; a scalar gain broadcasts over the paths
    delay = [[0.5, 3.0], [-0.125, 0.0], [7.75, 7.75]]
    got = get(amd.stream.propagate(xd, delay=delay, gain=0.5, sfo_ppm=[20.0, -20.0, 0.0], cfo=[0.01, -0.02, 0.0]))
    want = pc.propagate_host(x, delay=[[W(v) for v in row] for row in delay], gain=[[0.5, 0.5]],
                             sfo=[pc.sfo_word(v) for v in (20.0, -20.0, 0.0)],
                             fcw=[int(round(v * 2.0 ** 64)) for v in (0.01, -0.02, 0.0)])
    assert (bits(got) == bits(want)).all()
    # device tensors: a float delay is rounded on the device, an int64 one is words
    dt = torch.tensor(delay, dtype=torch.float64, device="cuda")
    gt = torch.tensor([[1.0, 0.5j]] * 3, dtype=torch.complex64, device="cuda")
    a = get(amd.stream.propagate(xd, delay=dt, gain=gt))
    b = get(amd.stream.propagate(xd, delay=words([[W(v) for v in row] for row in delay], 3, 2), gain=gt))
    want = pc.propagate_host(x, delay=[[W(v) for v in row] for row in delay], gain=[[1.0, 0.5j]])
    assert (bits(a) == bits(want)).all() and (bits(b) == bits(want)).all()
    # an sfo_ppm tensor likewise: floats are parts per million, int64 is words
    ppm = [20.0, -40.0, 244.0]
    sw = [pc.sfo_word(v) for v in ppm]
    a = get(amd.stream.propagate(xd, delay=0.5, sfo_ppm=torch.tensor(ppm, dtype=torch.float32, device="cuda")))
    b = get(amd.stream.propagate(xd, delay=0.5, sfo_ppm=words(sw, 3)))
    want = pc.propagate_host(x, delay=W(0.5), sfo=sw)
    assert (bits(a) == bits(want)).all() and (bits(b) == bits(want)).all()
    with pytest.raises(TypeError):
        amd.stream.propagate(xd, sfo_ppm=torch.tensor([1, 2, 3], dtype=torch.int32, device="cuda"))
    # one row in, one row out; a length of its own; a window
    got = get(amd.stream.propagate(xd[1], delay=0.5, length=1200, in_first=40, first_sample=30))
    assert got.shape == (1200,)
    assert (bits(got) == bits(pc.propagate_host(x[1], 1200, delay=W(0.5), in_first=40, first_sample=30))).all()
    # the host-side refusals
    with pytest.raises(ValueError):
        amd.stream.propagate(xd, delay=[0.0, 1.0], gain=[1.0, 0.5, 0.25])
    with pytest.raises(ValueError):
        amd.stream.propagate(xd, delay=40000.0)
    with pytest.raises(ValueError):
        amd.stream.propagate(xd, sfo_ppm=300.0)
    with pytest.raises(amd.LoraError, match="in and out overlap"):
        amd.stream.propagate(xd, out=xd)
    with pytest.raises(ValueError):
        amd.stream.propagate(xd, table=np.zeros((256, 3), np.float32))
