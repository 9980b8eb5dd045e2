"""GPU: self-describing frames on the device (lora_phy_amd.codec.encode_frame / decode_frame /
decode_header over csrc/lora_codec.hip, LoRaMod.work_frame) and the frame gather
(stream.gather_frames_device over csrc/lora_gather.hip) against their numpy restatement,
tests/frame_checker.py, which tests/test_frame_checker.py checks on the CPU.  Integer work and
copies: every comparison is exact."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import frame_checker as fc  # noqa: E402

SENT8, SENT16, SENT32 = 0xA5, 0xBEEF, 0x7F7F7F7F
FIELDS = ("status", "nbytes", "rdd", "has_crc", "nsym", "errors")


@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import lora_phy_amd

    return lora_phy_amd


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def fields(res):
    return {k: getattr(res, k).cpu().numpy() for k in FIELDS}


def same_fields(res, want, key):
    got = fields(res)
    for k, h in zip(FIELDS, fc.FIELDS):
        assert np.array_equal(got[k], want[h]), (key, k, got[k], want[h])


def sizes(sf):
    return np.array([0, 1, 2, 3, 4, 5, sf, 16, 17, 255])


# ---------------------------------------------------------------------------------
# The codec over the grid: SF 7-12 x rdd 0-4 x crc 0/1, ten sizes as the rows of one batch
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("sf", range(7, 13))
def test_codec_equals_the_checker_over_the_grid(amd, sf):
    nbytes = sizes(sf)
    for rdd in range(5):
        for crc in (0, 1):
            key = (sf, rdd, crc)
            pay = np.random.default_rng(100 * sf + 10 * rdd + crc).integers(0, 256, (len(nbytes), 255)).astype(np.uint8)
            want_sym, want_nsym = fc.encode_batch(pay, nbytes, sf, rdd, crc)
            sym, nsym = amd.codec.encode_frame(dev(pay, np.uint8), dev(nbytes, np.int32), sf, rdd, crc=bool(crc))
            assert sym.shape == want_sym.shape == (len(nbytes), amd.codec.frame_symbols(sf, rdd, 255, bool(crc)))
            assert np.array_equal(sym.cpu().numpy(), want_sym), key
            assert np.array_equal(nsym.cpu().numpy(), want_nsym), key
            # every row is a whole frame followed by zeros: decoded with and without its own count
            want = fc.decode_batch(want_sym, sf, max_bytes=255)
            assert (want["status"] == fc.OK).all() and np.array_equal(want["nbytes"], nbytes), key
            for avail in (None, nsym):
                res = amd.codec.decode_frame(sym, sf, avail=avail)
                assert res.payload.shape == (len(nbytes), 255)
                same_fields(res, want, key)
                got = res.payload.cpu().numpy()
                assert np.array_equal(got, want["payload"]), key
                for f, n in enumerate(nbytes):
                    assert np.array_equal(got[f, :n], pay[f, :n]) and not got[f, n:].any(), (key, f)
            head = amd.codec.decode_header(sym, sf)
            assert head.payload is None
            same_fields(head, fc.decode_batch(want_sym, sf), key)
            # one symbol fewer than the frame has
            res = amd.codec.decode_frame(sym, sf, avail=nsym - 1)
            same_fields(res, fc.decode_batch(want_sym, sf, want_nsym - 1, 255), key)
            assert (res.status.cpu().numpy() == fc.SHORT).all() and not res.payload.cpu().numpy().any(), key


# ---------------------------------------------------------------------------------
# Lanes per frame, more than one workgroup, damaged frames
# ---------------------------------------------------------------------------------
# the encoder gives a frame 2^lg lanes by the symbols of a max_bytes frame, the decoder by
# max_bytes + 2 bytes, 64 at the most: max_bytes on both sides of the decoder's steps, and 300
# frames so that every group size spans workgroups (256 >> lg frames each)
@pytest.mark.parametrize("max_bytes", [0, 1, 2, 3, 6, 7, 14, 15, 30, 31, 62, 63, 100])
def test_group_sizes_and_damaged_frames(amd, max_bytes):
    F = 300
    rng = np.random.default_rng(max_bytes)
    sf, rdd, crc = 7 + max_bytes % 6, max_bytes % 5, (max_bytes >> 1) & 1
    nbytes = rng.integers(0, max_bytes + 1, F)
    nbytes[:2] = (0, max_bytes)
    pay = rng.integers(0, 256, (F, max_bytes)).astype(np.uint8)
    want_sym, want_nsym = fc.encode_batch(pay, nbytes, sf, rdd, crc)
    S = want_sym.shape[1]
    # strided rows inside sentinels, outputs that start as garbage
    d_pay = torch.full((F, max_bytes + 3), SENT8, dtype=torch.uint8, device="cuda")
    d_pay[:, :max_bytes] = dev(pay, np.uint8)
    d_sym = torch.full((F, S + 5), SENT16, dtype=torch.int32, device="cuda").to(torch.uint16)
    d_nsym = torch.full((F,), SENT32, dtype=torch.int32, device="cuda")
    sym, nsym = amd.codec.encode_frame(d_pay[:, :max_bytes], dev(nbytes, np.int32), sf, rdd, crc=bool(crc),
                                       out=d_sym[:, :S], out_nsym=d_nsym)
    assert sym.data_ptr() == d_sym.data_ptr() and nsym is d_nsym
    h = d_sym.cpu().numpy()
    assert np.array_equal(h[:, :S], want_sym) and (h[:, S:] == SENT16).all()
    assert np.array_equal(d_nsym.cpu().numpy(), want_nsym)
    # damage: every third frame gets three random data symbols (bits above sf set too; one wrong
    # symbol is one bit per codeword, which the longer codes correct), every third two random
    # header symbols, the rest stay whole; avail varies around the frame's own count
    bad = want_sym.copy()
    for f in range(F):
        if f % 3 == 1 and want_nsym[f] > 8:
            for k in rng.integers(8, want_nsym[f], 3):
                bad[f, k] = rng.integers(0, 1 << 16)
        elif f % 3 == 2:
            for k in rng.choice(8, 2, replace=False):
                bad[f, k] = rng.integers(0, 1 << 16)
    avail = want_nsym + rng.integers(-1, 3, F)
    avail[5:9] = (-4, 0, 7, 1 << 20)
    h_sym = np.full((F, S + 5), SENT16, np.uint16)
    h_sym[:, :S] = bad
    wide = max_bytes + 4
    pay_buf = torch.full((F, wide + 3), SENT8, dtype=torch.uint8, device="cuda")
    out = amd.codec.FrameResult(payload=pay_buf[:, 1:1 + wide],
                                **{k: torch.full((F,), SENT32, dtype=torch.int32, device="cuda") for k in FIELDS})
    for av, mb in ((avail, wide), (None, wide), (avail, max_bytes), (avail, max(max_bytes - 1, 0))):
        want = fc.decode_batch(bad, sf, av, mb)
        if mb == wide:
            res = amd.codec.decode_frame(dev(h_sym, np.uint16)[:, :S], sf, None if av is None else dev(av, np.int32),
                                         max_bytes=mb, out=out)
            assert res is out
            base = pay_buf.cpu().numpy()
            assert (base[:, 0] == SENT8).all() and (base[:, 1 + wide:] == SENT8).all()
        else:
            res = amd.codec.decode_frame(dev(h_sym, np.uint16)[:, :S], sf, None if av is None else dev(av, np.int32),
                                         max_bytes=mb)
        same_fields(res, want, (max_bytes, mb))
        assert np.array_equal(res.payload.cpu().numpy(), want["payload"]), (max_bytes, mb)
    st = fc.decode_batch(bad, sf, avail, wide)["status"]
    if max_bytes >= 14:  # the batch holds whole, damaged and short frames
        assert {fc.OK, fc.SHORT, fc.HEADER} <= set(st.tolist()) and (not crc or fc.CRC in st)
    head = amd.codec.decode_header(dev(h_sym, np.uint16)[:, :S], sf, dev(avail, np.int32))
    same_fields(head, fc.decode_batch(bad, sf, avail), max_bytes)


def test_random_symbols_decode_as_the_checker_says(amd):
    """Rows of random uint16 symbols: nearly every header is bad, the few that pass state some
    length; whatever comes out equals the checker."""
    for sf in (7, 9, 12):
        sym = np.random.default_rng(sf).integers(0, 1 << 16, (4000, 40)).astype(np.uint16)
        head = amd.codec.decode_header(dev(sym, np.uint16), sf)
        want = fc.decode_batch(sym, sf)
        same_fields(head, want, sf)
        assert (want["status"] == fc.HEADER).sum() > 3900
        keep = np.flatnonzero(want["status"] == fc.OK)[:64]
        if len(keep):
            res = amd.codec.decode_frame(dev(sym[keep], np.uint16), sf)
            full = fc.decode_batch(sym[keep], sf, max_bytes=res.payload.shape[1])
            same_fields(res, full, sf)
            assert np.array_equal(res.payload.cpu().numpy(), full["payload"])


def test_single_frame_and_default_width(amd):
    pay = bytes(range(40, 60))
    sym = fc.encode_frame(pay, 8, 2, 1)
    got, nsym = amd.codec.encode_frame(dev(list(pay), np.uint8), None, 8, "4/6")
    assert got.shape == (len(sym),) and np.array_equal(got.cpu().numpy(), sym) and int(nsym.cpu()[0]) == len(sym)
    res = amd.codec.decode_frame(got, 8)
    assert res.payload.shape == (amd.codec.frame_capacity(8, len(sym)),)
    assert bytes(res.payload.cpu().numpy()[:20]) == pay and int(res.status.cpu()[0]) == fc.OK
    with pytest.raises(ValueError):
        amd.codec.decode_frame(got, 8, max_bytes=256)
    with pytest.raises(amd.LoraError):
        amd.codec.decode_frame(got, 6)
    with pytest.raises((TypeError, ValueError)):
        amd.codec.decode_frame(got, 8, avail=torch.zeros(1, dtype=torch.int64, device="cuda"))


def test_no_allocation_per_call_with_outputs_given(amd):
    F, n, sf = 64, 20, 9
    pay = torch.randint(0, 256, (F, n), dtype=torch.uint8, device="cuda")
    nb = torch.randint(0, n + 1, (F,), dtype=torch.int32, device="cuda")
    sym, nsym = amd.codec.encode_frame(pay, nb, sf, 3)
    res = amd.codec.decode_frame(sym, sf, nsym, max_bytes=n)
    head = amd.codec.decode_header(sym, sf)
    torch.cuda.synchronize()
    stats = torch.cuda.memory_stats()["allocation.all.allocated"]
    for _ in range(3):
        amd.codec.encode_frame(pay, nb, sf, 3, out=sym, out_nsym=nsym)
        amd.codec.decode_frame(sym, sf, nsym, max_bytes=n, out=res)
        amd.codec.decode_header(sym, sf, out=head)
    torch.cuda.synchronize()
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == stats
    keep = torch.arange(n, device="cuda") < nb[:, None]
    assert bool((res.status == 0).all() & (res.nbytes == nb).all() & (res.payload == pay * keep).all())


# ---------------------------------------------------------------------------------
# Modulated frames
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("sf,ovs", [(7, 1), (8, 2)])
def test_work_frame_is_silent_after_each_frame(amd, sf, ovs):
    """LoRaMod.work_frame: each row is its frame's modulation, then zero samples; demodulated
    and decoded with the lengths the headers state, the payloads come back."""
    F, max_bytes, cr = 6, 12, 2
    rng = np.random.default_rng(sf)
    pay = rng.integers(0, 256, (F, max_bytes)).astype(np.uint8)
    nbytes = np.array([0, 12, 5, 1, 12, 7])
    mod = amd.LoRaMod(sf, ovs=ovs, cr=cr)
    iq = mod.work_frame(pay, nbytes)
    want_sym, want_nsym = fc.encode_batch(pay, nbytes, sf, cr, 1)
    step = (1 << sf) * ovs
    assert iq.shape == (F, (want_sym.shape[1] + 2) * step)
    whole = amd.modulate(dev(want_sym, np.uint16), sf, ovs).cpu().numpy()
    h = iq.cpu().numpy()
    for f in range(F):
        end = (2 + want_nsym[f]) * step
        assert np.array_equal(h[f, :end], whole[f, :end]) and not h[f, end:].any(), f
    res = amd.LoRaDemod(sf, osr=ovs).work_frames(iq)
    dec = amd.codec.decode_frame(res.symbols, sf, avail=dev(want_nsym, np.int32), max_bytes=max_bytes)
    assert (dec.status.cpu().numpy() == fc.OK).all() and np.array_equal(dec.nsym.cpu().numpy(), want_nsym)
    got = dec.payload.cpu().numpy()
    for f, n in enumerate(nbytes):
        assert np.array_equal(got[f, :n], pay[f, :n]) and not got[f, n:].any()
    # the headers alone, with no length given, state the same
    head = amd.codec.decode_header(res.symbols, sf)
    assert np.array_equal(head.nbytes.cpu().numpy(), nbytes) and (head.rdd.cpu().numpy() == cr).all()


# ---------------------------------------------------------------------------------
# The frame gather
# ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stream_samples():
    rng = np.random.default_rng(11)
    return (rng.standard_normal(30001) + 1j * rng.standard_normal(30001)).astype(np.complex64)


# cuts on both sides of a workgroup's 2048 samples, odd and even, and one of several workgroups
@pytest.mark.parametrize("cut", [1, 2, 7, 640, 2047, 2048, 2049, 5000])
def test_gather_equals_the_host_model(amd, stream_samples, cut):
    flat = stream_samples
    L = len(flat)
    rng = np.random.default_rng(cut)
    # odd and even offsets with lengths from 0 to the cut and beyond; empty slots; a frame that
    # ends exactly on the last sample, one that would run over it, one that starts on it
    at = list(rng.integers(0, L - cut, 24)) + [0, 1, 2, 3, -1, -1, L - cut, L - cut + 1, L - 1, L, L + 5]
    ln = list(rng.integers(0, cut + 1, 24)) + [cut, cut, cut - 1, cut - 1, cut, 0, cut, cut, cut, cut, 3]
    ln[0], ln[1], ln[2], ln[3] = 0, 1, cut, cut + 9
    want = fc.gather_host(flat, at, ln, cut)
    d_flat = dev(flat, np.complex64)
    got = amd.stream.gather_frames_device(d_flat, dev(at, np.int64), dev(ln, np.int64), cut)
    assert got.shape == want.shape and got.data_ptr() % 16 == 0 and (len(at) < 2 or got.stride(0) % 2 == 0)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), cut
    # a stream that starts on an odd sample (8-byte aligned only), into sentinel-filled output
    pitch = cut + 4 + (cut & 1)
    buf = torch.full((len(at), pitch), complex(7, 7), dtype=torch.complex64, device="cuda")
    got = amd.stream.gather_frames_device(d_flat[1:], dev(at, np.int64), dev(ln, np.int64), cut, out=buf[:, :cut])
    assert got.data_ptr() == buf.data_ptr()
    h = buf.cpu().numpy()
    assert np.array_equal(h[:, :cut].view(np.uint32), fc.gather_host(flat[1:], at, ln, cut).view(np.uint32)), cut
    assert (h[:, cut:] == complex(7, 7)).all()


def test_gather_from_strided_rows(amd, stream_samples):
    """[R, L] rows with a pitch: slot indices count along the flat stream the rows lie in, and a
    frame may end on the tensor's very last sample."""
    R, L, rs, cut = 3, 4001, 4100, 900
    flat = stream_samples[:(R - 1) * rs + L]
    rows = dev(stream_samples[:R * rs], np.complex64).view(R, rs)[:, :L]
    starts = np.array([[0, 17, L - cut], [1, 2000, L - cut], [-1, 3, L - cut]])
    at = np.where(starts < 0, -1, starts + rs * np.arange(R)[:, None]).reshape(-1)
    ln = np.array([cut, 0, cut, 13, cut - 1, cut, cut, 500, cut])
    got = amd.stream.gather_frames_device(rows, dev(at, np.int64), dev(ln, np.int64), cut)
    assert np.array_equal(got.cpu().numpy(), fc.gather_host(flat, at, ln, cut))
    assert at[-1] + cut == len(flat)
    one = amd.stream.gather_frames_device(rows[0], dev(at[:3], np.int64), dev(ln[:3], np.int64), cut)
    assert np.array_equal(one.cpu().numpy(), fc.gather_host(flat[:L], at[:3], ln[:3], cut))
    none = amd.stream.gather_frames_device(rows, dev([], np.int64), dev([], np.int64), cut)
    assert none.shape == (0, cut)


def test_a_gathered_frame_demodulates_as_the_frame_alone(amd):
    """Frames of different lengths back to back in one stream: each slot's DemodResult equals
    plan.run on that frame zero-padded to the cut, bit for bit - the neighbours' samples are not
    in it."""
    sf, cr, max_bytes = 7, 1, 16
    pay = np.random.default_rng(5).integers(0, 256, (3, max_bytes)).astype(np.uint8)
    nbytes = np.array([0, 16, 5])
    sym, nsym = fc.encode_batch(pay, nbytes, sf, cr, 1)
    assert list(nsym) == [13, 38, 18]
    step = 1 << sf
    frames = [amd.modulate(dev(sym[f, :nsym[f]], np.uint16), sf) for f in range(3)]
    lens = np.array([len(x) for x in frames])
    assert np.array_equal(lens, (2 + nsym) * step)
    stream = torch.cat(frames)
    at = np.concatenate([[0], np.cumsum(lens)[:-1]])
    cut = (2 + int(nsym.max())) * step
    got = amd.stream.gather_frames_device(stream, dev(at, np.int64), dev(lens, np.int64), cut)
    padded = torch.zeros((3, cut), dtype=torch.complex64, device="cuda")
    for f in range(3):
        padded[f, :lens[f]] = frames[f]
    assert torch.equal(got, padded)
    plan = amd.LoRaDemod(sf).plan
    a, b = plan.run(got), plan.run(padded)
    torch.cuda.synchronize()
    assert np.array_equal(a.symbols.cpu().numpy(), b.symbols.cpu().numpy())
    for name in ("sync", "cfo", "time_offset", "max_amp"):
        x, y = getattr(a, name).cpu().numpy(), getattr(b, name).cpu().numpy()
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), name
    dec = amd.codec.decode_frame(a.symbols, sf, dev(nsym, np.int32), max_bytes=max_bytes)
    assert (dec.status.cpu().numpy() == fc.OK).all()
    for f, n in enumerate(nbytes):
        assert np.array_equal(dec.payload.cpu().numpy()[f, :n], pay[f, :n])
