"""CPU: the drop-in scenarios of tests/dropin_script.py put their inputs where they claim.

tests/test_gpu_dropin_paths.py compares the drop-in with the oracle's answers on these
scenarios; it proves something only if the oracle's answers are the ones the scenario is
about - a refusal where the scratch is short, a non-zero sync word and cfo, other symbols at
another osr, 255 symbols for the long frame, sample counts on both sides of the staging's
limits.  Those conditions are checked here, without a GPU, and so is the comparison itself:
it accepts what a correct driver prints and rejects single wrong values.
"""
import json

import numpy as np
import pytest

from tests import dropin_script as ds


@pytest.mark.parametrize("name", sorted(ds.SCENARIOS))
def test_scenario_is_complete_and_deterministic(name, tmp_path):
    """One expectation per script line (no call is left out of the comparison), every demodulate
    has its whole output array expected, and a second build from the seeds is identical."""
    scn = ds.build(name)
    assert len(scn.lines) == len(scn.expect) > 0
    for line, want in zip(scn.lines, scn.expect):
        assert line.split()[0] == want["kind"]
        assert "state" in want
        if want["kind"] in ("ldemod", "demod"):
            assert {"ret", "sync", "cfo_bits", "toff_bits", "symbols"} <= set(want)
            assert want["symbols"][max(want["ret"], 0):] == [ds.SYM_FILL] * (len(want["symbols"]) - max(want["ret"], 0))
        if want["kind"] in ("lmod", "mod", "comp"):
            assert "out" in want
    again = ds.SCENARIOS[name]()
    assert again.lines == scn.lines and again.data() == scn.data()
    script, data, _ = scn.write(str(tmp_path))
    assert open(script).read().splitlines() == scn.lines
    assert open(data, "rb").read() == scn.data()


def test_A_every_configuration_has_a_nonzero_sync_and_cfo():
    configs = ds.build("A").facts["configs"]
    assert [(c["sf"], c["hann"]) for c in configs] == [(sf, h) for sf in range(2, 13) for h in (False, True)]
    for c in configs:
        N = 1 << c["sf"]
        assert [a["count"] for a in c["answers"]] == [N - 1, N, 2 * N, 3 * N, 9 * N + 5, 4 * N + 1]
        assert [len(a["oracle"][0]) for a in c["answers"]] == [0, 1, 0, 1, (9 * N + 5) // N - 2, 2]
        assert any(a["oracle"][1] != 0 and a["oracle"][2] not in (0, 0x80000000) for a in c["answers"]), c
        assert not any(a["refused"] for a in c["answers"])
        assert sum(a["peak"] > 1.0 for a in c["answers"]) == 1  # the rescale path, scratch long enough
        assert c["answers"][-1]["oracle"][1] != 0


def test_B_oracle_refuses_exactly_the_short_scratch_frames():
    cases = ds.build("B").facts["cases"]
    assert len(cases) == 2 * 3 * 4
    one_up = float(np.nextafter(np.float32(1), np.float32(2)))
    assert sorted({c["peak"] for c in cases if c["peak"] >= 1.0}) == [1.0, one_up, 3.0]
    seen = set()
    for c in cases:
        syms, sync, cfo_bits, toff_bits = c["oracle"]
        short = c["scratch_len"] < c["count"]
        seen.add((c["peak"] > 1.0, short, c["scratch_len"] == 0))
        if c["peak"] > 1.0 and short:
            assert c["refused"]
            assert len(syms) == 0 and sync == 0 and cfo_bits == 0 and toff_bits == 0, c
        else:
            assert not c["refused"]
            assert len(syms) > 0 and cfo_bits != 0, c
    assert seen == {(big, short, null) for big in (False, True) for short, null in
                    ((False, False), (True, False), (True, True))}


def test_C_other_osr_gives_other_symbols():
    facts = ds.build("C").facts["osr2"]
    assert [f["sf"] for f in facts] == [8, 12]
    for f in facts:
        assert len(f["at2"]) == f["nsym"]
        assert not np.array_equal(f["at2"], f["at1"][:f["nsym"]]), f


def test_D_five_workspaces_at_once():
    scn = ds.build("D")
    kinds = [line.split()[0] for line in scn.lines]
    assert kinds[:5] == ["linit"] * 5 and ds.SLOTS == 4
    assert scn.expect[scn.facts["fifth_init"]]["state"]["borrowed"] is False
    frames = [line.split()[3] for line in scn.lines if line.startswith("ldemod")]
    assert len(set(frames)) == len(frames) == 15  # distinct frames


def test_E_long_frame_is_255_symbols_past_the_slot():
    for info in ds.build("E").facts["long"]:
        assert info["count"] == 257 * 4096 > ds.SLOT_SAMPLES
        assert len(info["oracle"][0]) == 255 and not info["refused"]


def test_F_sample_counts_straddle_the_staging_limits():
    calls = ds.build("F").facts["calls"]
    for c in calls:
        assert c["samples"] == (c["nsym"] + 2) * (1 << c["sf"]) * c["osr"]
        assert c["queue"] == (c["samples"] <= ds.MOD_SAMPLES and c["nsym"] <= ds.MOD_SYMS)
    by = {(c["sf"], c["osr"], c["nsym"]): c["samples"] for c in calls}
    assert by[(12, 1, 510)] == 2097152 == ds.MOD_SAMPLES and by[(12, 1, 511)] > ds.MOD_SAMPLES
    assert (2, 1, 65536) in by and (2, 1, 65537) in by and ds.MOD_SYMS == 65536
    # past the limits: first use, a larger call (the buffer grows), a smaller one (reused)
    past = [c["samples"] for c in calls if not c["queue"]]
    assert past[1] < past[0] < past[2] > past[3]


def test_G_error_returns_and_ignored_window():
    scn = ds.build("G")
    assert scn.facts["errors"] == [-1, -1, -1]
    h = scn.facts["hann_ignored"]
    assert h["ret"] == 6 == h["hann"][0]
    # with the window applied the answer would differ: a drop-in that applied it would show
    assert (h["got"]["cfo_bits"], h["got"]["toff_bits"]) != (ds.bits(h["hann"][3]), ds.bits(h["hann"][4]))
    # the short estimate leaves the metrics of the one before
    i = next(k for k, line in enumerate(scn.lines) if line.startswith("est") and int(line.split()[3]) < 256)
    assert all(scn.expect[i][k] == scn.expect[i - 1][k] for k in ("cfo_bits", "toff_bits"))
    assert scn.expect[i - 1]["cfo_bits"] != scn.expect[i - 2]["cfo_bits"]


def test_H_cycles_the_frame_lengths():
    scn = ds.build("H")
    counts = [int(line.split()[4]) for line in scn.lines if line.startswith("ldemod")]
    assert len(counts) == 150 and counts[:4] == [128, 256, 384, 40 * 128 + 5] and counts[4:8] == counts[:4]


def satisfy(want, states):
    """A device state that passes check_state(want)."""
    st = {"slot": -1, "shared_plan": False, "shared_aql": False, "aql": False, "aql_status": 0, "samples": 0,
          "plan_osr": 0}
    for key, v in want.items():
        if key == "borrowed":
            st["slot"] = 0 if v else -1
        elif key == "own_queue_or_hip":
            st["aql"] = True
        elif key == "samples_min":
            st["samples"] = v
        elif key not in ("slot_same_as", "slot_differs_from"):
            st[key] = v
    if "slot_same_as" in want:
        st["slot"] = states[want["slot_same_as"]]["slot"]
    if "slot_differs_from" in want:
        taken = {states[i]["slot"] for i in want["slot_differs_from"]}
        st["slot"] = min(v for v in range(ds.SLOTS) if v not in taken)
    return st


def render(scn, out_path):
    """What a correct driver prints for the scenario (a state that satisfies each call's
    checks) - for checking `compare` itself on the CPU."""
    lines, n_out, states = [], 0, []
    with open(out_path, "wb") as fh:
        for i, want in enumerate(scn.expect):
            row = {"op": i}
            for key, v in want.items():
                if key == "out":
                    row.update(out_off=n_out, out_count=len(v))
                    fh.write(v.tobytes())
                    n_out += len(v)
                elif key != "state":
                    row[key] = v
            row["state"] = None if want["state"] is None else satisfy(want["state"], states)
            states.append(row["state"])
            lines.append(json.dumps(row))
    lines.append(json.dumps({"ops": len(scn.expect), "dropin_status": 0}))
    return "\n".join(lines) + "\n"


def test_compare_accepts_a_correct_driver_and_rejects_wrong_values(tmp_path):
    """The comparison on what a correct driver would print for G, B and D, then with one symbol,
    one metric bit, one sample bit, one state field and the runtime's status changed."""
    for name in ("G", "B", "D"):
        scn = ds.build(name)
        out = str(tmp_path / f"{name}.bin")
        good = render(scn, out)
        assert ds.compare(scn, good, out) == len(scn.lines)
        rows = [json.loads(line) for line in good.splitlines()]

        def changed(i, key, value):
            r = [dict(row) for row in rows]
            r[i][key] = value
            return "\n".join(json.dumps(row) for row in r) + "\n"

        i = next(k for k, w in enumerate(scn.expect) if w["kind"] in ("ldemod", "demod") and w["ret"] > 0)
        syms = list(rows[i]["symbols"])
        syms[0] ^= 1
        for bad in (changed(i, "symbols", syms), changed(i, "cfo_bits", rows[i]["cfo_bits"] ^ 1),
                    changed(i, "sync", rows[i]["sync"] ^ 0x10), changed(i, "ret", rows[i]["ret"] - 1),
                    changed(i, "state", dict(rows[i]["state"], shared_aql=not rows[i]["state"]["shared_aql"])),
                    changed(len(rows) - 1, "dropin_status", 5)):
            with pytest.raises(AssertionError):
                ds.compare(scn, bad, out)
        # a refused call that wrote a symbol after all
        k = next((k for k, w in enumerate(scn.expect) if w["kind"] in ("ldemod", "demod") and w["ret"] <= 0), None)
        if k is not None:
            syms = list(rows[k]["symbols"])
            syms[0] = 0
            with pytest.raises(AssertionError):
                ds.compare(scn, changed(k, "symbols", syms), out)
    scn = ds.build("G")
    out = str(tmp_path / "G.bin")
    raw = bytearray(open(out, "rb").read())
    raw[len(raw) // 2] ^= 1
    open(out, "wb").write(bytes(raw))
    with pytest.raises(AssertionError):
        ds.compare(scn, render(scn, str(tmp_path / "G2.bin")), out)
