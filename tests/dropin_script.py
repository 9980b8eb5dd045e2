"""Scenarios for tests/native/seq_dropin: scripted sequences of drop-in calls that take the
workspaces of include/lora_mi355x_phy.hpp past the load-time runtime's limits (four slots of
1 M samples, shared osr-1 plans, a modulator staging of 2 M samples / 64 K symbols).

Each scenario is built from seeds: the IQ and symbol payloads (one data file), the script
(one text line per call, format in tests/native/seq_dropin.cpp) and, per call, what the CPU
oracle (oracle.pyoracle.Oracle) says the call must return - symbols, sync word, cfo and
time_offset bit patterns, modulated or compensated samples - together with what the
caller-visible device state must read after it.  Nothing here needs a GPU:
tests/test_dropin_script.py checks on the CPU that the oracle puts every scenario's inputs
where the scenario claims, tests/test_gpu_dropin_paths.py runs the scripts on the MI355X.

The rules this module restates itself (the oracle's ctypes wrapper starts every call from
zeroed outputs, so it cannot tell "wrote zero" from "wrote nothing"):
* lora_demodulate returns 0 before writing anything when the frame's maximum is > 1 and the
  scratch is null or shorter than the frame (LoRaDemod.cpp:68-71);
* demodulate returns -1 before writing anything for a partial symbol, fewer than two symbols
  or a short symbol buffer (phy.cpp:186-190);
* estimate_offsets leaves the metrics alone without a whole symbol (phy.cpp:87);
* init zeroes the metrics and stores the sync word (phy.cpp:31-34); the window applies only
  with a window buffer (phy.cpp:97,223); modulate sends the workspace's current sync word,
  which demodulate overwrites (phy.cpp:72-73,236).
"""
from __future__ import annotations

import functools
import json
import os

import numpy as np

from oracle.pyoracle import Oracle

# the driver's sentinels (tests/native/seq_dropin.cpp)
SYM_FILL = 0xA5A5
SYNC_FILL = 0xEE
CFO_FILL = -1234.5
TOFF_FILL = 4321.25
# the runtime's limits (csrc/lora_phy_dropin.hip: kSlots, kSlotSamples, kModSamples, kModSyms)
SLOTS = 4
SLOT_SAMPLES = 1 << 20
MOD_SAMPLES = 1 << 21
MOD_SYMS = 1 << 16


def bits(v) -> int:
    return int(np.float32(v).view(np.uint32))


def from_bits(b) -> float:
    return float(np.uint32(b).view(np.float32))


@functools.lru_cache(maxsize=1)
def oracle() -> Oracle:
    return Oracle()


def peak(x) -> float:
    """The demodulator's max_amp: the largest |re| or |im| (LoRaDemod.cpp:61-67)."""
    x = np.asarray(x, np.complex64)
    return float(max(np.abs(x.real).max(), np.abs(x.imag).max())) if len(x) else 0.0


def with_peak(x, value) -> np.ndarray:
    """x scaled so that its maximum is about `value` (complex64)."""
    return (np.asarray(x, np.complex64) * np.float32(value / peak(x))).astype(np.complex64)


def with_exact_peak(x, value) -> np.ndarray:
    """x scaled to a maximum of 0.5, then one real part set to `value` exactly."""
    y = with_peak(x, 0.5)
    y.real[len(y) // 2 + 3] = np.float32(value)
    assert peak(y) == float(np.float32(value))
    return y


def noise(rng, n, sigma=1.0) -> np.ndarray:
    return (sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)


def chirp_frame(rng, sf, osr, nsamples, sigma, *, sync=0x12, top=0.9):
    """A modulated frame covering nsamples (sync pair first), AWGN of sigma, dechirped as the
    reference's callers do before lora_demodulate (e2e_chain_test.cpp:84-93), cut to nsamples
    and scaled to a maximum of `top`."""
    O = oracle()
    step = (1 << sf) * osr
    total = -(-nsamples // step)
    syms = rng.integers(0, 1 << sf, max(total - 2, 0)).astype(np.uint16)
    x = O.lora_modulate(syms, sf, osr, 125000, 1.0, sync)
    x = O.dechirp((x + noise(rng, len(x), sigma)).astype(np.complex64), sf, osr)
    return with_peak(x[:nsamples], top)


class Script:
    """One scenario: script lines, payload, and per call the expectation and the state checks."""

    def __init__(self, name):
        self.name = name
        self.lines = []
        self.expect = []   # per call: dict of exact values (plus "state": checks, "out": samples)
        self.facts = {}    # what tests/test_dropin_script.py checks about the inputs
        self._chunks = []
        self._bytes = 0
        self._seen = {}
        self.legacy = {}
        self.api = {}

    # ---- payload ----------------------------------------------------------------------------
    def _put(self, arr, dtype):
        arr = np.ascontiguousarray(np.asarray(arr, dtype))
        key = (id(arr), dtype)
        if key in self._seen:
            return self._seen[key][1]
        pad = -self._bytes % 8
        if pad:
            self._chunks.append(b"\0" * pad)
            self._bytes += pad
        off = self._bytes // arr.dtype.itemsize
        self._chunks.append(arr.tobytes())
        self._bytes += arr.nbytes
        self._seen[key] = (arr, off)  # (the array is kept: its id stays its own)
        return off

    def data(self) -> bytes:
        return b"".join(self._chunks)

    def _op(self, line, expect, state):
        expect["state"] = state
        self.lines.append(line)
        self.expect.append(expect)
        return len(self.lines) - 1

    # ---- legacy helpers ---------------------------------------------------------------------
    def linit(self, w, sf, hann, max_samples, scratch=True, state=None):
        self.legacy[w] = dict(sf=sf, hann=bool(hann), max_samples=max_samples, scratch=scratch)
        return self._op(f"linit {w} {sf} {int(hann)} {max_samples} {'buf' if scratch else 'null'}",
                        {"kind": "linit", "N": 1 << sf}, state)

    def lfree(self, w):
        del self.legacy[w]
        return self._op(f"lfree {w}", {"kind": "lfree"}, RELEASED)

    def ldemod(self, w, osr, x, state=None):
        cfg = self.legacy[w]
        x = np.ascontiguousarray(np.asarray(x, np.complex64))
        scratch_len = cfg["max_samples"] if cfg["scratch"] else 0
        syms, sync, cfo, toff = oracle().lora_demodulate(x, cfg["sf"], osr, cfg["hann"], scratch_len=scratch_len)
        out = np.full(len(x) // ((1 << cfg["sf"]) * osr) + 2, SYM_FILL, np.uint16)
        refused = peak(x) > 1.0 and scratch_len < len(x)  # LoRaDemod.cpp:68-71
        if refused:
            want = {"ret": 0, "sync": SYNC_FILL, "cfo_bits": bits(CFO_FILL), "toff_bits": bits(TOFF_FILL)}
        else:
            out[:len(syms)] = syms
            want = {"ret": len(syms), "sync": sync, "cfo_bits": bits(cfo), "toff_bits": bits(toff)}
        want.update(kind="ldemod", symbols=[int(v) for v in out])
        i = self._op(f"ldemod {w} {osr} {self._put(x, np.complex64)} {len(x)}", want, state)
        return i, dict(oracle=(syms, sync, bits(cfo), bits(toff)), refused=refused, peak=peak(x),
                       scratch_len=scratch_len, count=len(x))

    def lmod(self, sf, osr, bw, amplitude, sync, syms, queue):
        syms = np.ascontiguousarray(np.asarray(syms, np.uint16))
        out = oracle().lora_modulate(syms, sf, osr, bw, amplitude, sync)
        return self._op(f"lmod {sf} {osr} {bw} {bits(amplitude)} {sync} {self._put(syms, np.uint16)} {len(syms)}",
                        {"kind": "lmod", "ret": len(out), "queue": queue, "out": out}, None)

    # ---- workspace API ----------------------------------------------------------------------
    def init(self, w, sf, osr, bw, hann, window_buffer, sync, state=None):
        self.api[w] = dict(sf=sf, osr=osr, bw=bw, hann=bool(hann and window_buffer), sync=sync, cfo_bits=0,
                           toff_bits=0)
        window0 = (0.0 if hann else 1.0) if window_buffer else -1.0  # (the driver's fill: no buffer given)
        return self._op(f"init {w} {sf} {osr} {bw} {int(hann)} {int(window_buffer)} {sync}",
                        {"kind": "init", "ret": 0, "sync": sync, "cfo_bits": 0, "toff_bits": 0,
                         "window0": bits(window0)}, state)

    def demod(self, w, x, cap=None, state=None):
        m = self.api[w]
        x = np.ascontiguousarray(np.asarray(x, np.complex64))
        step = (1 << m["sf"]) * m["osr"]
        total = len(x) // step
        cap = max(total - 2, 0) if cap is None else cap
        r, syms, sync, cfo, toff = oracle().api_demodulate(x, m["sf"], m["osr"], m["hann"], bw=m["bw"], cap=cap)
        out = np.full(max(cap, total) + 2, SYM_FILL, np.uint16)
        if r < 0:
            want = {"ret": -1, "sync": m["sync"], "cfo_bits": bits(CFO_FILL), "toff_bits": bits(TOFF_FILL)}
            m.update(cfo_bits=bits(CFO_FILL), toff_bits=bits(TOFF_FILL))  # (the driver's pre-fill stays)
        else:
            out[:r] = syms
            m.update(sync=sync, cfo_bits=bits(cfo), toff_bits=bits(toff))
            want = {"ret": r, "sync": sync, "cfo_bits": bits(cfo), "toff_bits": bits(toff)}
        want.update(kind="demod", symbols=[int(v) for v in out])
        return self._op(f"demod {w} {self._put(x, np.complex64)} {len(x)} {cap}", want, state), r

    def est(self, w, x, state=None):
        m = self.api[w]
        x = np.ascontiguousarray(np.asarray(x, np.complex64))
        if len(x) // ((1 << m["sf"]) * m["osr"]) > 0:  # phy.cpp:87
            cfo, toff = oracle().estimate_offsets(x, m["sf"], m["osr"], m["hann"])
            m.update(cfo_bits=bits(cfo), toff_bits=bits(toff))
        return self._op(f"est {w} {self._put(x, np.complex64)} {len(x)}",
                        {"kind": "est", "sync": m["sync"], "cfo_bits": m["cfo_bits"], "toff_bits": m["toff_bits"]},
                        state)

    def comp(self, w, x, state=None):
        m = self.api[w]
        x = np.ascontiguousarray(np.asarray(x, np.complex64))
        out = oracle().compensate_offsets(x, m["sf"], m["osr"], from_bits(m["cfo_bits"]), from_bits(m["toff_bits"]))
        return self._op(f"comp {w} {self._put(x, np.complex64)} {len(x)}",
                        {"kind": "comp", "sync": m["sync"], "cfo_bits": m["cfo_bits"], "toff_bits": m["toff_bits"],
                         "out": out}, state)

    def mod(self, w, syms, cap, state=None):
        m = self.api[w]
        syms = np.ascontiguousarray(np.asarray(syms, np.uint16))
        need = (len(syms) + 2) * (1 << m["sf"]) * m["osr"]
        if need > cap:  # phy.cpp:74
            want = {"kind": "mod", "ret": -1, "out": np.zeros(0, np.complex64)}
        else:
            out = oracle().lora_modulate(syms, m["sf"], m["osr"], m["bw"], 1.0, m["sync"])
            want = {"kind": "mod", "ret": need, "out": out}
        return self._op(f"mod {w} {self._put(syms, np.uint16)} {len(syms)} {cap}", want, state)

    def destroy(self, w):
        del self.api[w]
        return self._op(f"destroy {w}", {"kind": "destroy"}, None)

    # ---- files ------------------------------------------------------------------------------
    def write(self, directory):
        """script.txt and data.bin under `directory`; returns (script, data, out) paths."""
        script = os.path.join(directory, "script.txt")
        data = os.path.join(directory, "data.bin")
        with open(script, "w") as fh:
            fh.write("\n".join(self.lines) + "\n")
        with open(data, "wb") as fh:
            fh.write(self.data())
        return script, data, os.path.join(directory, "out.bin")


# ---- the device state a call must leave (detail::device_state, printed by the driver) ---------
# Keys: borrowed (slot >= 0), slot_same_as / slot_differs_from (call indices), own_queue_or_hip
# (a queue of its own, or none with aql_status saying why), samples_min, and exact values for
# shared_plan, shared_aql, aql, aql_status, samples, plan_osr.
BORROWED = dict(borrowed=True, shared_plan=True, shared_aql=True, aql=True, aql_status=0, samples=SLOT_SAMPLES,
                plan_osr=1)
RELEASED = dict(borrowed=False, shared_plan=False, shared_aql=False, aql=False, samples=0)


def check_state(got, want, states, where):
    if want is None:
        assert got is None, where
        return
    assert got is not None, where
    for key, v in want.items():
        if key == "borrowed":
            assert (got["slot"] >= 0) == v, (where, key, got)
            if v:
                assert got["slot"] < SLOTS, (where, got)
            else:
                assert got["slot"] == -1, (where, got)
        elif key == "slot_same_as":
            assert got["slot"] == states[v]["slot"], (where, key, got, states[v])
        elif key == "slot_differs_from":
            assert all(got["slot"] != states[i]["slot"] for i in v), (where, key, got)
        elif key == "own_queue_or_hip":
            assert (got["aql"] and not got["shared_aql"] and got["aql_status"] == 0) or \
                (not got["aql"] and got["aql_status"] != 0), (where, key, got)
        elif key == "samples_min":
            assert got["samples"] >= v, (where, key, got)
        else:
            assert got[key] == v, (where, key, got)


def compare(scn, stdout, out_path):
    """Every line the driver printed against the scenario's expectation, exactly; the samples
    it wrote as uint32 views.  Returns the number of calls compared (all of them)."""
    rows = [json.loads(line) for line in stdout.splitlines() if line.startswith("{")]
    assert rows, stdout
    last = rows.pop()
    assert last == {"ops": len(scn.expect), "dropin_status": 0}, last
    assert len(rows) == len(scn.expect)
    produced = np.fromfile(out_path, np.complex64) if os.path.exists(out_path) else np.zeros(0, np.complex64)
    states = []
    for i, (got, want) in enumerate(zip(rows, scn.expect)):
        where = f"scenario {scn.name} call {i}: {scn.lines[i]}"
        assert got["op"] == i and got["kind"] == want["kind"], where
        states.append(got["state"])
        for key, v in want.items():
            if key == "state":
                check_state(got["state"], v, states, where)
            elif key == "out":
                assert got["out_count"] == len(v), (where, got["out_count"], len(v))
                samples = produced[got["out_off"]:got["out_off"] + got["out_count"]]
                assert len(samples) == len(v), where
                bad = np.flatnonzero(samples.view(np.uint32) != v.view(np.uint32))
                assert bad.size == 0, (where, f"{bad.size} words differ, first at {bad[0]}")
            else:
                assert got[key] == v, (where, key, got[key], v)
        assert set(got) - {"op", "out_off", "out_count"} == set(want) - {"out"}, (where, sorted(got), sorted(want))
    return len(rows)


# ---- scenarios ------------------------------------------------------------------------------

def scenario_A():
    """Every SF and window on a borrowed slot, one workspace re-initialised each time."""
    s = Script("A")
    rng = np.random.default_rng(0xA0)
    s.facts["configs"] = []
    k = 0
    for sf in range(2, 13):
        for hann in (False, True):
            N = 1 << sf
            s.linit(0, sf, hann, 9 * N + 5, True, state=BORROWED)
            answers = []
            for j, n in enumerate((N - 1, N, 2 * N, 3 * N, 9 * N + 5, 4 * N + 1)):
                kind = (k + j) % 4
                if n == 9 * N + 5:
                    x = chirp_frame(rng, sf, 1, n, (0.0, 0.3)[k % 2])
                elif n == 4 * N + 1:
                    x = chirp_frame(rng, sf, 1, n, 0.3, sync=0x5A, top=2.5)  # rescaled, scratch long enough
                elif kind == 3:
                    x = with_peak(noise(rng, n), 0.9)
                else:
                    x = chirp_frame(rng, sf, 1, n, (0.0, 0.3, 2.0)[kind])
                _, info = s.ldemod(0, 1, x, state=BORROWED)
                answers.append(info)
            s.facts["configs"].append(dict(sf=sf, hann=hann, answers=answers))
            if k % 2 == 0:
                s.lfree(0)
            k += 1
    s.lfree(0)
    return s


def scenario_B():
    """Short scratch: frames that need rescaling without room for it return 0, untouched."""
    s = Script("B")
    rng = np.random.default_rng(0xB0)
    s.facts["cases"] = []
    for sf, hann in ((7, False), (10, True)):
        N = 1 << sf
        count = 6 * N
        base = chirp_frame(rng, sf, 1, count, 0.3)
        frames = [with_exact_peak(base, v) for v in (1.0, np.nextafter(np.float32(1), np.float32(2)), 3.0)]
        for max_samples, scratch in ((count, True), (count - 1, True), (0, False)):
            s.linit(0, sf, hann, max_samples, scratch, state=BORROWED)
            for x in frames:
                _, info = s.ldemod(0, 1, x, state=BORROWED)
                s.facts["cases"].append(info)
            _, info = s.ldemod(0, 1, chirp_frame(rng, sf, 1, 4 * N + 7, 0.3, sync=0x34), state=BORROWED)
            s.facts["cases"].append(info)
        s.lfree(0)
    return s


def scenario_C():
    """osr per call on one workspace: shared plan -> own plan -> shared plan, slot kept."""
    s = Script("C")
    rng = np.random.default_rng(0xC0)
    s.facts["osr2"] = []
    for w, (sf, osrs, nsym) in enumerate(((8, (1, 2, 1, 4, 3, 1), 6), (12, (1, 2, 1), 3))):
        N = 1 << sf
        i0 = s.linit(w, sf, False, (nsym + 2) * N * max(osrs), True, state=BORROWED)
        for osr in osrs:
            x = chirp_frame(rng, sf, osr, (nsym + 2) * N * osr, 0.3)
            _, info = s.ldemod(w, osr, x, state=dict(borrowed=True, slot_same_as=i0, shared_plan=osr == 1,
                                                     shared_aql=True, aql=True, plan_osr=osr,
                                                     samples_min=SLOT_SAMPLES))
            if osr == 2:
                at1 = oracle().lora_demodulate(x, sf, 1, False)[0]
                s.facts["osr2"].append(dict(sf=sf, nsym=nsym, at2=info["oracle"][0], at1=at1))
        s.lfree(w)
    return s


def scenario_D():
    """Past the four slots: a fifth workspace at once, interleaved frames, a freed slot reused."""
    s = Script("D")
    rng = np.random.default_rng(0xD0)
    sf, N = 9, 512
    count = 8 * N
    # (own buffers, stream and queue; the osr-1 plan is still the runtime's: ensure_plan)
    own = dict(borrowed=False, shared_plan=True, shared_aql=False, own_queue_or_hip=True, plan_osr=1,
               samples_min=count)
    inits, spec = {}, {}
    for w in range(5):
        spec[w] = dict(BORROWED, slot_differs_from=[inits[v] for v in range(w)]) if w < 4 else own
        inits[w] = s.linit(w, sf, False, count, True, state=spec[w])
        spec[w] = dict(spec[w], slot_same_as=inits[w])
        spec[w].pop("slot_differs_from", None)

    def frame(j):
        return chirp_frame(rng, sf, 1, count, (0.0, 0.3, 2.0)[j % 3], sync=(0x12, 0x34, 0x5A, 0xC3)[j % 4],
                           top=(0.9, 2.5)[j % 5 == 0])

    j = 0
    for _ in range(2):
        for w in (0, 3, 1, 4, 2):
            s.ldemod(w, 1, frame(j), state=spec[w])
            j += 1
    s.lfree(1)
    spec[5] = dict(BORROWED, slot_same_as=inits[1])  # the one free slot
    inits[5] = s.linit(5, sf, True, count, True, state=spec[5])
    for w in (5, 4, 0, 5):
        s.ldemod(w, 1, frame(j), state=spec[w])
        j += 1
    for w in (3, 0, 5, 4, 2):
        s.lfree(w)
    s.linit(6, sf, False, count, True, state=BORROWED)
    s.ldemod(6, 1, frame(j), state=BORROWED)
    s.lfree(6)
    s.facts["fifth_init"] = inits[4]
    return s


def scenario_E():
    """Past 1 M samples: at init (no slot), and by growth out of a borrowed slot."""
    s = Script("E")
    rng = np.random.default_rng(0xE0)
    sf, N = 12, 4096
    long_n = 257 * N
    xl = chirp_frame(rng, sf, 1, long_n, 0.3)
    xl_big = with_peak(xl, 2.5)
    own = dict(borrowed=False, shared_plan=True, shared_aql=False, own_queue_or_hip=True, plan_osr=1,
               samples=long_n)
    s.facts["long"] = []
    # (i) too large for a slot at init
    s.linit(0, sf, False, (1 << 20) + 4096, True, state=own)
    _, info = s.ldemod(0, 1, xl_big, state=own)
    s.facts["long"].append(info)
    s.ldemod(0, 1, chirp_frame(rng, sf, 1, 3 * N, 0.3), state=own)
    s.lfree(0)
    # (ii) a slot at init, then a frame larger than the slot's buffers
    i0 = s.linit(1, sf, True, 3 * N, True, state=BORROWED)
    grown = dict(BORROWED, slot_same_as=i0, samples=long_n)
    _, info = s.ldemod(1, 1, xl, state=grown)
    s.facts["long"].append(info)
    s.ldemod(1, 1, chirp_frame(rng, sf, 1, 3 * N, 0.0), state=grown)
    s.lfree(1)
    s.linit(1, sf, True, 3 * N, True, state=BORROWED)
    s.ldemod(1, 1, chirp_frame(rng, sf, 1, 3 * N, 2.0), state=BORROWED)
    s.lfree(1)
    return s


def scenario_F():
    """lora_modulate at the staging's limits: the queue up to 2 M samples and 64 K symbols, the
    thread-local device buffer past either (grown, then reused)."""
    s = Script("F")
    rng = np.random.default_rng(0xF0)

    def syms(n, sf):
        v = rng.integers(0, 1 << sf, n).astype(np.uint16)
        v[::7] = rng.integers(1 << sf, 1 << 16, len(v[::7])).astype(np.uint16)  # symbols >= N
        return v

    calls = [  # sf, osr, bw, amplitude, sync, symbols, on the queue
        (12, 1, 125000, 1.0, 0x12, 510, True),     # exactly 2^21 samples
        (12, 1, 125000, 0.5, 0x34, 511, False),    # one symbol more
        (2, 1, 125000, 1.0, 0x12, 65536, True),    # exactly 2^16 symbols
        (2, 1, 125000, 1.0, 0x12, 65537, False),   # (the 511-symbol call's buffer is large enough)
        (7, 1, 125000, 1.0, 0x12, 5, True),
        (12, 2, 250000, 1.7, 0xAB, 300, False),    # larger than the buffer: grown
        (2, 1, 125000, -0.25, 0xC3, 65537, False),  # reused
        (9, 2, 250000, 0.8, 0x5A, 10, True),
        (12, 1, 500000, 1.0, 0x12, 511, False),
        (8, 1, 500000, 1.0, 0x12, 7, True),
    ]
    s.facts["calls"] = []
    for sf, osr, bw, amp, sync, n, queue in calls:
        i = s.lmod(sf, osr, bw, amp, sync, syms(n, sf), queue)
        s.facts["calls"].append(dict(sf=sf, osr=osr, nsym=n, queue=queue, samples=s.expect[i]["ret"]))
    return s


def scenario_G():
    """Workspace API: buffers grown by demodulate, compensate_offsets (2x) and
    estimate_offsets, the error returns, and re-init with other parameters."""
    s = Script("G")
    rng = np.random.default_rng(0x60)
    O = oracle()
    sf, osr = 7, 2
    step = (1 << sf) * osr
    s4, s12 = (rng.integers(0, 1 << sf, n).astype(np.uint16) for n in (4, 12))
    x4, x12 = ((O.lora_modulate(v, sf, osr, 125000, 1.0, 0x34) + noise(rng, (len(v) + 2) * step, 0.25))
               .astype(np.complex64) for v in (s4, s12))
    api = dict(borrowed=False, shared_plan=False, shared_aql=False, aql=False, plan_osr=osr)

    def st(samples, **kw):
        return dict(api, samples=samples, **kw)

    s.init(0, sf, osr, 125000, True, True, 0x34, state=st(0))
    s.demod(0, x4, state=st(len(x4)))
    s.comp(0, x12, state=st(2 * len(x12)))
    s.est(0, x12, state=st(2 * len(x12)))
    s.est(0, x12[:step - 56], state=st(2 * len(x12)))  # no whole symbol: metrics unchanged
    s.demod(0, x12, state=st(2 * len(x12)))
    errors = []
    errors.append(s.demod(0, x12[:len(x12) - 100], state=st(2 * len(x12)))[1])   # a partial symbol
    s.demod(0, x4, state=st(2 * len(x12)))
    errors.append(s.demod(0, x12[:step], state=st(2 * len(x12)))[1])            # one symbol
    s.demod(0, x12, state=st(2 * len(x12)))
    errors.append(s.demod(0, x12, cap=len(x12) // step - 3, state=st(2 * len(x12)))[1])  # cap = total - 3
    s.demod(0, x4, cap=9, state=st(2 * len(x12)))
    s.mod(0, s12, len(x12) - 1, state=st(2 * len(x12)))  # phy.cpp:74
    s.mod(0, s12, len(x12), state=st(2 * len(x12)))      # (with the sync word the last demodulate found)
    s.comp(0, x4, state=st(2 * len(x12)))
    s.facts["errors"] = errors
    # re-init: SF10, osr 1, 250 kHz, Hann requested without a window buffer (so: no window)
    sf2 = 10
    v = rng.integers(0, 1 << sf2, 6).astype(np.uint16)
    y = (O.lora_modulate(v, sf2, 1, 250000, 1.0, 0x5A) + noise(rng, 8 << sf2, 0.25)).astype(np.complex64)
    api = dict(api, plan_osr=1)
    s.init(0, sf2, 1, 250000, True, False, 0x12, state=st(0))
    _, r = s.demod(0, y, state=st(len(y)))
    s.facts["hann_ignored"] = dict(ret=r, got=s.expect[-1], hann=O.api_demodulate(y, sf2, 1, True, bw=250000))
    s.est(0, y[:5 << sf2], state=st(len(y)))
    s.comp(0, y[:(3 << sf2) + 9], state=st(len(y)))
    s.mod(0, v, len(y), state=st(len(y)))
    # re-init: SF9 at 500 kHz, the window buffer back
    sf3 = 9
    v = rng.integers(0, 1 << sf3, 5).astype(np.uint16)
    z = (O.lora_modulate(v, sf3, 1, 500000, 1.0, 0xC3) + noise(rng, 7 << sf3, 0.25)).astype(np.complex64)
    s.init(0, sf3, 1, 500000, False, True, 0x12, state=st(0))
    s.demod(0, z, state=st(len(z)))
    s.mod(0, v, len(z), state=st(len(z)))
    s.destroy(0)
    # a second workspace after the first is gone
    s.init(1, sf, osr, 125000, True, True, 0x34, state=dict(api, plan_osr=osr, samples=0))
    s.demod(1, x12, state=dict(api, plan_osr=osr, samples=len(x12)))
    s.destroy(1)
    return s


def scenario_H():
    """A long mixed run on one workspace: the 64-packet queue wraps at varying packet counts."""
    s = Script("H")
    rng = np.random.default_rng(0x70)
    sf, N = 7, 128
    lens = (N, 2 * N, 3 * N, 40 * N + 5)
    s.linit(0, sf, False, max(lens), True, state=BORROWED)
    for i in range(150):
        n = lens[i % 4]
        if i % 11 == 3:
            x = with_peak(noise(rng, n), 0.9)
        else:
            x = chirp_frame(rng, sf, 1, n, (0.0, 0.3, 2.0)[i % 3], sync=(0x12, 0x34, 0xC3)[(i // 4) % 3],
                            top=(0.9, 2.5)[i % 10 == 7])
        s.ldemod(0, 1, x, state=BORROWED)
    s.lfree(0)
    return s


SCENARIOS = {"A": scenario_A, "B": scenario_B, "C": scenario_C, "D": scenario_D, "E": scenario_E,
             "F": scenario_F, "G": scenario_G, "H": scenario_H}


@functools.lru_cache(maxsize=None)
def build(name) -> Script:
    return SCENARIOS[name]()
