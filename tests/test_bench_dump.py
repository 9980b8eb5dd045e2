"""bench.py --dump-outputs on the host: float32 .npy files named after the outputs, and an
output beyond its share of the size cap written as a fixed, seeded sample."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    import bench as b

    return b


def test_small_outputs_are_written_whole(bench, tmp_path):
    last = {"symbols": torch.arange(12, dtype=torch.int32).reshape(3, 4), "cfo": torch.tensor([0.25, -1.5, 3.0])}
    bench.dump_outputs(str(tmp_path / "d"), last)
    assert sorted(os.listdir(tmp_path / "d")) == ["cfo.npy", "symbols.npy"]
    s, c = np.load(tmp_path / "d" / "symbols.npy"), np.load(tmp_path / "d" / "cfo.npy")
    assert s.dtype == c.dtype == np.float32
    assert np.array_equal(s, np.arange(12, dtype=np.float32).reshape(3, 4))
    assert np.array_equal(c, np.float32([0.25, -1.5, 3.0]))
    bench.dump_outputs(str(tmp_path / "d"), last, rank=2)
    assert np.array_equal(np.load(tmp_path / "d" / "symbols.rank2.npy"), s)


def test_large_output_is_a_fixed_sample_within_the_cap(bench, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4096)  # 2 arrays: 512 float32 elements each
    big = torch.arange(100_000, dtype=torch.int32).reshape(1000, 100)
    small = torch.ones(7)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"symbols": big, "cfo": small})
    a, b = np.load(tmp_path / "a" / "symbols.npy"), np.load(tmp_path / "b" / "symbols.npy")
    assert a.shape == (512,) and a.dtype == np.float32 and np.array_equal(a, b)
    # distinct elements of the output, in their order (the values are their own flat indices)
    assert np.all(np.diff(a) > 0) and a[-1] < 100_000
    assert np.load(tmp_path / "a" / "cfo.npy").shape == (7,)
    total = sum(os.path.getsize(tmp_path / "a" / f) - 128 for f in os.listdir(tmp_path / "a"))
    assert total <= 4096
