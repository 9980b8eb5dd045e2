"""CPU: the three filter banks refuse a bad call with the same code and the same text as when
tests/golden/bank_error_texts.json was recorded.  The cases are the refusals that
tests/test_channel_capi.py, test_resample_capi.py, test_raw_capi.py and test_synth_capi.py construct,
plus calls that break two rules at once (names with ``&``), which pin the order of the checks.
The banks share their host-side rules (csrc/lora_bank.h); this is what holds "same check, same
precedence, same text" across them.  No case reaches a HIP call.

``python -m tests.test_bank_error_texts`` (the repository root and the package's folder on
PYTHONPATH) records the file again from the library that is built."""
import ctypes as C
import json
import os

import pytest

from lora_phy_amd import _capi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bank_error_texts.json")
FORMATS = {"cs16": (_capi.LORA_IQ_CS16, 4), "cs8": (_capi.LORA_IQ_CS8, 2), "cu8": (_capi.LORA_IQ_CU8, 2)}
STEPS = (C.c_int32 * 2)(1, -1)
GAINS = (C.c_float * 2)(1.0, 0.5)
A = 4096  # a made-up non-NULL address: no case gets as far as following a pointer


def ptr(v):
    return v if v is None or not isinstance(v, int) else C.c_void_p(v)


# ---- the callers: keyword defaults are a legal call, a case overrides some ----------------
DOWN = dict(iq=A, format=None, scale=1.0, rows=1, row_len=1000, row_stride=1000, first=0, taps=A, nco=A, period=5,
            st=STEPS, channels=2, out=A)
INT_BASE = dict(DOWN, ntaps=65, decim=8, out_stride=200)             # 117 outputs per row
RAT_BASE = dict(DOWN, ntaps=49, interp=3, decim=8, out_stride=400)   # 369 outputs per row
SYN_BASE = dict(inp=A, rows=1, chan_len=100, in_stride=100, first=0, taps=A, ntaps=65, interp=8, nco=A, period=5,
                st=STEPS, g=GAINS, channels=2, out=A, out_stride=736, format=None, inv=32768.0)  # 736 outputs


def call_integer(lib, a):
    tail = (a["rows"], a["row_len"], a["row_stride"], a["first"], ptr(a["taps"]), a["ntaps"], a["decim"],
            ptr(a["nco"]), a["period"], a["st"], a["channels"], ptr(a["out"]), a["out_stride"], 0, None)
    if a["format"] is None:
        return lib.lora_channelize_batch(ptr(a["iq"]), *tail)
    return lib.lora_channelize_raw_batch(ptr(a["iq"]), a["format"], a["scale"], *tail)


def call_rational(lib, a):
    tail = (a["rows"], a["row_len"], a["row_stride"], a["first"], ptr(a["taps"]), a["ntaps"], a["interp"], a["decim"],
            ptr(a["nco"]), a["period"], a["st"], a["channels"], ptr(a["out"]), a["out_stride"], 0, None)
    if a["format"] is None:
        return lib.lora_resample_channelize_batch(ptr(a["iq"]), *tail)
    return lib.lora_resample_channelize_raw_batch(ptr(a["iq"]), a["format"], a["scale"], *tail)


def call_synth(lib, a):
    head = (ptr(a["inp"]), a["rows"], a["chan_len"], a["in_stride"], a["first"], ptr(a["taps"]), a["ntaps"],
            a["interp"], ptr(a["nco"]), a["period"], a["st"], a["g"], a["channels"], ptr(a["out"]))
    if a["format"] is None:
        return lib.lora_synthesize_batch(*head, a["out_stride"], 0, None)
    return lib.lora_synthesize_raw_batch(*head, a["format"], a["inv"], a["out_stride"], 0, None)


# ---- the cases ---------------------------------------------------------------------------
DOWN_CASES = {
    "taps=NULL": dict(taps=None), "nco=NULL": dict(nco=None), "steps=NULL": dict(st=None), "out=NULL": dict(out=None),
    "iq=NULL": dict(iq=None),
    "rows=-1": dict(rows=-1), "row_len=-1": dict(row_len=-1), "row_stride=-1": dict(row_stride=-1),
    "out_stride=-1": dict(out_stride=-1), "first=-1": dict(first=-1),
    "period=0": dict(period=0), "period=4097": dict(period=4097),
    "channels=0": dict(channels=0), "channels=33": dict(channels=33),
    "row_stride<row_len": dict(rows=2, row_stride=999),
    "grid": dict(rows=1 << 40, row_stride=1000),
    # two rules at once
    "ntaps=0 & channels=33": dict(ntaps=0, channels=33),
    "taps=NULL & rows=-1": dict(taps=None, rows=-1),
    "period=0 & channels=0": dict(period=0, channels=0),
    "row_stride<row_len & out_stride<W": dict(rows=2, row_stride=999, out_stride=1),
    "out_stride<W & grid": dict(rows=1 << 40, out_stride=1),
    "grid & iq=NULL": dict(rows=1 << 40, iq=None),
}
INT_CASES = dict(DOWN_CASES, **{
    "ntaps=0": dict(ntaps=0), "ntaps=513": dict(ntaps=513), "ntaps=-3": dict(ntaps=-3),
    "decim=0": dict(decim=0), "decim=65": dict(decim=65),
    "row_len=2^31": dict(row_len=1 << 31, row_stride=1 << 31),
    "out_stride<W": dict(out_stride=116),
    "ntaps=0 & decim=0": dict(ntaps=0, decim=0),
    "decim=65 & period=0": dict(decim=65, period=0),
    "channels=33 & row_len=2^31": dict(channels=33, row_len=1 << 31, row_stride=1 << 31),
})
RAT_CASES = dict(DOWN_CASES, **{
    "interp=0": dict(interp=0), "interp=17": dict(interp=17, decim=32), "interp=-2": dict(interp=-2),
    "decim=0": dict(decim=0), "decim=257": dict(decim=257), "decim=-8": dict(decim=-8),
    "interp>decim": dict(interp=9, decim=8), "interp=2,decim=1": dict(interp=2, decim=1),
    "ntaps=0": dict(ntaps=0), "ntaps=4097": dict(ntaps=4097, interp=16, decim=16), "ntaps=-3": dict(ntaps=-3),
    "phase taps>512": dict(ntaps=3 * 512 + 1), "phase taps>512,interp=1": dict(ntaps=513, interp=1),
    "row_len=2^31": dict(row_len=1 << 31, row_stride=1 << 31, out_stride=1 << 31),
    "out_stride<W": dict(out_stride=368),
    "interp=0 & decim=0": dict(interp=0, decim=0),
    "decim=257 & interp>decim": dict(interp=16, decim=257),
    "interp>decim & ntaps=0": dict(interp=9, decim=8, ntaps=0),
    "phase taps>512 & period=0": dict(ntaps=3 * 512 + 1, period=0),
    "channels=33 & row_len=2^31": dict(channels=33, row_len=1 << 31, row_stride=1 << 31, out_stride=1 << 31),
})
SYN_CASES = {
    "in=NULL": dict(inp=None), "taps=NULL": dict(taps=None), "nco=NULL": dict(nco=None), "steps=NULL": dict(st=None),
    "gains=NULL": dict(g=None), "out=NULL": dict(out=None),
    "rows=-1": dict(rows=-1), "chan_len=-1": dict(chan_len=-1), "in_stride=-1": dict(in_stride=-1),
    "out_stride=-1": dict(out_stride=-1), "first=-1": dict(first=-1),
    "interp=0": dict(interp=0), "interp=65": dict(interp=65), "interp=-2": dict(interp=-2),
    "ntaps=0": dict(ntaps=0), "ntaps=513": dict(ntaps=513), "ntaps=-3": dict(ntaps=-3),
    "period=0": dict(period=0), "period=4097": dict(period=4097),
    "channels=0": dict(channels=0), "channels=33": dict(channels=33),
    "chan_len*interp=2^31": dict(chan_len=1 << 28, in_stride=1 << 28),
    "chan_len=2^31": dict(chan_len=1 << 31, in_stride=1 << 31, interp=1),
    "in_stride<chan_len": dict(in_stride=99),
    "in_stride<chan_len,rows=2": dict(rows=2, channels=1, in_stride=99),
    "out_stride<W": dict(rows=2, out_stride=735),
    "grid": dict(rows=1 << 40, out_stride=736),
    # two rules at once
    "rows=-1 & channels=33": dict(rows=-1, channels=33),
    "interp=0 & ntaps=0": dict(interp=0, ntaps=0),
    "ntaps=513 & period=0": dict(ntaps=513, period=0),
    "in_stride<chan_len & out_stride<W": dict(rows=2, in_stride=99, out_stride=735),
    "out_stride<W & grid": dict(rows=1 << 40, out_stride=735),
    "grid & taps=NULL": dict(rows=1 << 40, out_stride=736, taps=None),
}


def raw_cases(size):
    """The raw down-converter entries' own rules, for a format of `size` bytes a sample."""
    cases = {"format=0": dict(format=0), "format=4": dict(format=4), "format=-1": dict(format=-1),
             "format=0,rows=0": dict(format=0, rows=0), "format=4,iq=NULL,rows=0": dict(format=4, iq=None, rows=0),
             "format=0 & taps=NULL": dict(format=0, taps=None)}
    for k in range(1, size):
        cases["iq+%d" % k] = dict(iq=A + k)
        cases["iq+%d,rows=0" % k] = dict(iq=A + k, rows=0)
    cases["iq+1 & ntaps=0"] = dict(iq=A + 1, ntaps=0)
    return cases


def entries():
    """{entry: (caller, defaults, cases)}"""
    syn_float = dict(SYN_CASES, **{"out+4": dict(out=A + 4), "out+4 & grid": dict(out=A + 4, rows=1 << 40),
                                   "out_stride<W & out+4": dict(rows=2, out_stride=735, out=A + 4)})
    e = {"lora_channelize_batch": (call_integer, INT_BASE, INT_CASES),
         "lora_resample_channelize_batch": (call_rational, RAT_BASE, RAT_CASES),
         "lora_synthesize_batch": (call_synth, SYN_BASE, syn_float)}
    # the rules after the format check do not look at the format: all of them for cs16, and for
    # the 8-bit formats the raw entries' own rules
    for name, (fmt, size) in FORMATS.items():
        full = name == "cs16"
        e["lora_channelize_raw_batch/" + name] = (call_integer, dict(INT_BASE, format=fmt),
                                                  dict(INT_CASES if full else {}, **raw_cases(size)))
        e["lora_resample_channelize_raw_batch/" + name] = (call_rational, dict(RAT_BASE, format=fmt),
                                                           dict(RAT_CASES if full else {}, **raw_cases(size)))
        syn = {"out+%d" % (size // 2): dict(out=A + size // 2),
               "out_stride<W & out+1": dict(rows=2, out_stride=735, out=A + 1),
               "format=0": dict(format=0), "format=4": dict(format=4), "format=-1": dict(format=-1),
               "format=0 & rows=-1": dict(format=0, rows=-1)}
        e["lora_synthesize_raw_batch/" + name] = (call_synth, dict(SYN_BASE, format=fmt),
                                                  dict(SYN_CASES if full else {}, **syn))
    return e


def run_case(entry, case):
    caller, base, cases = entries()[entry]
    lib = _capi.lib()
    code = caller(lib, dict(base, **cases[case]))
    return int(code), lib.lora_last_error().decode()


def record():
    rows = []
    for entry, (_, _, cases) in sorted(entries().items()):
        for case in cases:
            code, text = run_case(entry, case)
            assert code < 0 and text, (entry, case, code, text)
            rows.append({"entry": entry, "case": case, "code": code, "text": text})
    with open(GOLDEN, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    return rows


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_recorded_cases_are_the_cases_here():
    want = {(entry, case) for entry, (_, _, cases) in entries().items() for case in cases}
    rows = golden()
    assert {(r["entry"], r["case"]) for r in rows} == want and len(rows) == len(want)
    # every entry has calls that break two rules at once
    for entry in entries():
        assert sum(1 for r in rows if r["entry"] == entry and " & " in r["case"]) >= 2


@pytest.mark.parametrize("row", golden(), ids=lambda r: "%s:%s" % (r["entry"], r["case"]))
def test_refusal_code_and_text(row):
    code, text = run_case(row["entry"], row["case"])
    assert code == row["code"] == _capi.LORA_EINVAL
    assert text == row["text"] and text


if __name__ == "__main__":
    print(len(record()), "cases ->", GOLDEN)
