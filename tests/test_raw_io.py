"""CPU: raw capture files (lora_phy_amd.iq_io.write_raw, read_raw, iter_stream_raw): interleaved
integer I, Q pairs with no header, as the radios' tools write them."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

DTYPES = [(torch.int16, "<i2"), (torch.int8, "i1"), (torch.uint8, "u1")]
IDS = ["cs16", "cs8", "cu8"]


def capture(td, nd, L, seed):
    info = np.iinfo(np.dtype(nd))
    a = np.random.default_rng(seed).integers(info.min, info.max + 1, (L, 2)).astype(np.dtype(nd).newbyteorder("="))
    a[0], a[-1] = (info.min, info.max), (info.max, info.min)
    return torch.from_numpy(a)


@pytest.mark.parametrize("td,nd", DTYPES, ids=IDS)
def test_write_then_read_is_the_identity(tmp_path, td, nd):
    from lora_phy_amd import iq_io

    raw = capture(td, nd, 1000, 1)
    path = str(tmp_path / "capture.raw")
    assert iq_io.write_raw(path, raw) == 1000
    # the file is the interleaved little-endian components and nothing else
    assert np.array_equal(np.fromfile(path, dtype=nd), raw.numpy().reshape(-1))
    back = iq_io.read_raw(path, td)
    assert back.dtype == td and back.shape == (1000, 2) and back.device.type == "cpu" and torch.equal(back, raw)
    # slices smaller than the file, a slice that does not divide it, and max_samples
    assert torch.equal(iq_io.read_raw(path, td, slice_samples=7), raw)
    assert torch.equal(iq_io.read_raw(path, td, max_samples=333, slice_samples=100), raw[:333])
    assert iq_io.read_raw(path, td, max_samples=0).shape == (0, 2)
    # a strided view is written as its values
    assert iq_io.write_raw(path, raw[::3]) == 334 and torch.equal(iq_io.read_raw(path, td), raw[::3])
    with pytest.raises(ValueError):
        iq_io.write_raw(path, raw.reshape(-1))
    with pytest.raises(TypeError):
        iq_io.write_raw(path, raw.to(torch.int32))
    with pytest.raises(TypeError):
        iq_io.read_raw(path, torch.float32)


@pytest.mark.parametrize("td,nd", DTYPES, ids=IDS)
def test_a_trailing_unpaired_component_is_ignored(tmp_path, td, nd):
    from lora_phy_amd import iq_io

    raw = capture(td, nd, 50, 2)
    path = str(tmp_path / "odd.raw")
    np.concatenate([raw.numpy().reshape(-1), raw.numpy()[0, :1]]).astype(nd).tofile(path)
    assert torch.equal(iq_io.read_raw(path, td), raw)
    assert sum(len(t) for _, t in iq_io.iter_stream_raw(path, td, 20, 0)) == 50
    open(path, "wb").close()  # an empty file: no samples, no chunks
    assert iq_io.read_raw(path, td).shape == (0, 2) and list(iq_io.iter_stream_raw(path, td, 20, 5)) == []


@pytest.mark.parametrize("td,nd", DTYPES, ids=IDS)
def test_iter_stream_raw_offsets_and_overlaps(tmp_path, td, nd):
    """iter_stream's contract: tensor = file[offset : offset + chunk + overlap] for offset = 0,
    chunk, 2 chunk, ... while offset is inside the file; consecutive chunks share `overlap`
    samples; the last chunk, and only it, holds at most `chunk` samples."""
    from lora_phy_amd import iq_io

    raw = capture(td, nd, 1000, 3)
    path = str(tmp_path / "stream.raw")
    iq_io.write_raw(path, raw)
    for chunk, overlap in ((300, 50), (250, 0), (1000, 10), (999, 3), (2000, 100), (1, 0)):
        if chunk == 1:
            iq_io.write_raw(path, raw[:5])
        L = 5 if chunk == 1 else 1000
        got = list(iq_io.iter_stream_raw(path, td, chunk, overlap))
        assert [off for off, _ in got] == list(range(0, L, chunk))
        for off, t in got:
            assert t.dtype == td and t.dim() == 2 and torch.equal(t, raw[:L][off:off + chunk + overlap])
        assert len(got[-1][1]) <= chunk
        for (_, a), (_, b) in zip(got, got[1:]):
            assert torch.equal(a[chunk:chunk + overlap], b[:len(a) - chunk])
    for bad in ((0, 0), (10, -1)):
        with pytest.raises(ValueError):
            next(iq_io.iter_stream_raw(path, td, *bad))
