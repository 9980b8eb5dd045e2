"""GPU: awgn.sweep_receive_preamble (the detection-probability sweep of the preambled chain) on a
handful of frames well above the noise: every planted frame comes back with its payload and its
offset, with and without a fractional part; and the existing sweep's new ``cfo_bins`` shows what
the preamble is for - under three whole bins the plain chain returns no planted start."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def awgn():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from lora_phy_amd import awgn

    return awgn


@pytest.mark.parametrize("cfo", [0.0, 5.0, -3.25])
def test_every_frame_back_well_above_the_noise(awgn, cfo):
    recs = awgn.sweep_receive_preamble(7, [12.0], frames=8, max_bytes=6, cfo_bins=cfo, seed=5, noise_windows=1000,
                                       noise_batch_samples=1 << 18)
    r, noise = recs
    assert r["planted"] == 8 and r["cfo_bins"] == cfo and r["preamble"] == 8 and r["preamble_acc"] == 6
    assert r["returned_ok"] == 8 and r["cfo_right"] == 8 and r["found_at_planted"] == 8, r
    assert r["false_frames"] == 0 and r["candidates_dropped"] == 0, r
    assert noise["noise_only"] and noise["windows"] >= 1000 and noise["false_frames_ok"] == 0, noise


def test_the_plain_sweep_takes_an_offset_and_is_unchanged_without_one(awgn):
    a = awgn.sweep_receive_frames(7, [12.0], frames=8, max_bytes=6, seed=5)
    b = awgn.sweep_receive_frames(7, [12.0], frames=8, max_bytes=6, seed=5, cfo_bins=0.0)
    assert a == b and a[0]["returned_ok"] == 8
    off = awgn.sweep_receive_frames(7, [12.0], frames=8, max_bytes=6, seed=5, cfo_bins=3.0)
    assert off[0]["found_at_planted"] == 0, off  # every start moved by three chips
