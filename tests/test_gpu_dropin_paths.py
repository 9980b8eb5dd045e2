"""GPU: the C++ drop-in's workspace lifecycle past the load-time runtime's limits.

tests/test_gpu_dropin.py's callers all borrow one of the runtime's four slots, its shared
osr-1 plans and its queue, with frames of at most 1 M samples.  Here tests/native/seq_dropin
runs the scenarios of tests/dropin_script.py - one process per scenario, so state carries
from call to call - through every SF and window on a slot (A), the short-scratch refusal (B),
osr switched between calls (C), a fifth workspace at once (D), frames past 1 M samples at
init and by growth (E), lora_modulate on both sides of its staging's limits (F), the
workspace API's buffer growth, error returns and re-init (G) and a long mixed run that wraps
the queue (H).  Every call is compared with the CPU oracle exactly - integers, fp32 bit
patterns, uint32 views of the samples - and the caller-visible device state printed after
every call proves the branch was reached; the runtime's status must be 0.
(tests/test_dropin_script.py checks on the CPU that the inputs are where they should be.)
"""
import os
import subprocess

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import dropin_script as ds  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SEQ = os.path.join(HERE, "native", "seq_dropin")


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def run(cmd, cwd=None, timeout=100):
    return subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=timeout)


def play(name, tmp_path):
    assert os.path.exists(SEQ), "tests/native/seq_dropin not built (make -C lora-sdr-...-_amd)"
    scn = ds.build(name)
    script, data, out = scn.write(str(tmp_path))
    r = run([SEQ, script, data, out])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert ds.compare(scn, r.stdout, out) == len(scn.lines)


def test_A_every_sf_and_window_on_a_borrowed_slot(tmp_path):
    play("A", tmp_path)


def test_B_short_scratch_returns_zero_and_writes_nothing(tmp_path):
    play("B", tmp_path)


def test_C_osr_per_call_swaps_the_plan(tmp_path):
    play("C", tmp_path)


def test_D_fifth_workspace_past_the_slots(tmp_path):
    play("D", tmp_path)


def test_E_frames_past_one_million_samples(tmp_path):
    play("E", tmp_path)


def test_F_modulator_staging_limits(tmp_path):
    play("F", tmp_path)


def test_G_workspace_api_growth_errors_and_reinit(tmp_path):
    play("G", tmp_path)


def test_H_long_mixed_run_wraps_the_queue(tmp_path):
    play("H", tmp_path)
