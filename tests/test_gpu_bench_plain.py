"""bench.py's plain run and its options: a plain run prints the headline line alone,
`--dump-outputs DIR` writes the last timed step's outputs (identical from run to run and equal
to the transmitted symbols of the noiseless batch), and `--full` adds everything else the
benchmark measures to the same headline."""
import json
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES, DATA, STEPS = 96, 16, 4
SMALL = ["--gpus", "1", "--steps", str(STEPS), "--warmup", "1", "--frames", str(FRAMES), "--data-symbols", str(DATA),
         "--prewarm-ms", "0"]
HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus")


@pytest.fixture()
def run_bench(monkeypatch, capsys):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    import bench as b

    for name in ("LAUNCH", "PREWARM_MS", "STREAMS", "SYNC"):  # main() sets them from its arguments
        monkeypatch.setattr(b, name, getattr(b, name))

    def run(args):
        monkeypatch.setattr(sys, "argv", ["bench.py"] + args)
        capsys.readouterr()
        b.main()
        lines = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
        assert len(lines) == 1, lines
        return b, json.loads(lines[0])

    return run


def _load(d):
    return {n: np.load(os.path.join(d, n + ".npy")) for n in ("symbols", "sync", "cfo", "time_offset")}


def test_plain_run_is_the_headline_alone_and_dumps_its_outputs(run_bench, tmp_path):
    b, line = run_bench(SMALL + ["--dump-outputs", str(tmp_path / "a")])
    assert line["full"] is False
    assert line["metric"] == b.METRIC and line["unit"] == "Msymbols/s" and line["dtype"] == "f32"
    assert line["higher_is_better"] is True and line["steps"] == STEPS and line["n_gpus"] == 1
    assert line["ms_per_step"] > 0
    # value = data symbols per second of the timed steps
    assert line["value"] == pytest.approx(FRAMES * DATA / (line["ms_per_step"] * 1e-3) / 1e6, rel=1e-9)
    assert line["config"]["symbols_ok"] is True
    for moved in ("roofline", "cpu_baseline", "extra"):
        assert moved not in line
    for moved in ("stage_ms", "parity", "one_stream"):
        assert moved not in line["config"]
    a = _load(str(tmp_path / "a"))
    assert sorted(os.listdir(tmp_path / "a")) == ["cfo.npy", "symbols.npy", "sync.npy", "time_offset.npy"]
    assert all(v.dtype == np.float32 for v in a.values())
    assert a["symbols"].shape == (FRAMES, DATA) and a["sync"].shape == a["cfo"].shape == (FRAMES,)
    # the headline's batch: seeded symbols, noiseless - the outputs are the transmitted symbols
    tx, _ = b.make_input(7, FRAMES, DATA, 20251015, torch.device("cuda", 0))
    assert np.array_equal(a["symbols"], tx.numpy().astype(np.float32))
    assert np.all(a["sync"] == float(0x12))
    # the same arguments again: the same inputs, the same outputs, bit for bit
    run_bench(SMALL + ["--dump-outputs", str(tmp_path / "b")])
    bb = _load(str(tmp_path / "b"))
    for n in a:
        assert np.array_equal(a[n].view(np.uint32), bb[n].view(np.uint32)), n


def test_full_run_keeps_the_headline_and_adds_the_rest(run_bench, tmp_path):
    b, line = run_bench(SMALL + ["--full", "--no-cpu", "--sf12-frames", "8", "--channel-frames", "512",
                                 "--dump-outputs", str(tmp_path / "f")])
    assert line["full"] is True
    for k in HEADLINE_KEYS:
        assert k in line
    assert line["steps"] == STEPS and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(FRAMES * DATA / (line["ms_per_step"] * 1e-3) / 1e6, rel=1e-9)
    cfg = line["config"]
    assert cfg["symbols_ok"] is True and cfg["parity"]["parity_ok"] is True
    assert len(cfg["stage_ms"]) == 3 and cfg["one_stream"]["symbols_ok"] is True
    assert line["roofline"]["kernel"] == "k_spec_demod" and line["roofline"]["frac"] > 0
    extra = line["extra"]
    for k in ("fast_rotation_sf7", "sync_ff_sf7", "awgn_0db_sf7", "awgn_m10db_sf7", "hann_sf7", "long_frames_sf7",
              "osr2_sf7", "osr4_sf7", "api_sf7", "raw_sf7", "mod_sf7", "sf12", "fast_rotation_sf12",
              "awgn_m10db_sf12", "mod_sf12", "channels"):
        assert k in extra, k
    assert extra["sf12"]["parity"]["parity_ok"] is True and extra["sf12"]["symbols_ok"] is True
    assert extra["channels"]["symbols_ok_all_frames"] is True
    f = _load(str(tmp_path / "f"))
    tx, _ = b.make_input(7, FRAMES, DATA, 20251015, torch.device("cuda", 0))
    assert np.array_equal(f["symbols"], tx.numpy().astype(np.float32))
