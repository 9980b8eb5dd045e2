"""Time the down-converter banks on raw SDR samples (stream.Channelizer.run on int16, int8 and
uint8 [L, 2] tensors) beside the path they replace: stream.raw_to_complex in torch operations,
then the float kernel.  Both headline shapes on record - one stream of 32 Mi wideband samples
into 8 channels with 65 taps at decim 8 (tools/channel_time.py's bank) and with 385 taps at 5/96
(tools/resample_time.py's) - on one GPU, in one process.  A one-off measurement for DESIGN.md,
not part of bench.py.  Needs a HIP GPU.

For each bank and each of cs16, cs8 and cu8, the median (with the range) over ``--repeats``
device-event windows of ``--calls`` back-to-back calls on one stream after warm-up, the three
alternating so a drift of the machine shows in all:
  raw                   (a) Channelizer.run(raw, out=...): the one kernel, reading the integers
  convert_then_float    (b) raw_to_complex(raw), then Channelizer.run(x, out=...): the convert
                        pass's torch kernels and their complex64 result, then the float kernel
  float                 (c) Channelizer.run(x, out=...) on samples converted beforehand
``raw_below_convert_then_float``: (b)'s median minus (a)'s exceeds (b)'s own range over the
windows.  Before anything is timed (a)'s output is compared with (c)'s, bit for bit.
And once per format, (d): the host-to-device copy of the raw capture beside that of its complex64
form, both from pinned host memory into resident device tensors, the two alternating.

``--attach KEY=FILE`` (repeatable): store the JSON object of FILE under KEY, for what belongs to
the record but is measured by other commands in the same session - ``float_path_vs_parent``: the
float kernels' timings by tools/channel_time.py and tools/resample_time.py at this commit and at
its parent; ``load_loop_variants``: this tool's raw and float figures for another build of the
load loop.

usage: python tools/raw_time.py [--repeats 7] [--samples 33554432] [--attach key=f.json] [--out file.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lora-sdr-lightweight-standalone-library-_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--samples", type=int, default=1 << 25)
    ap.add_argument("--calls", type=int, default=5, help="calls per timed window")
    ap.add_argument("--attach", action="append", default=[], metavar="KEY=FILE",
                    help="store FILE's JSON object under KEY")
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch

    import channel_time as ct
    import resample_time as rt
    from lora_phy_amd import stream

    if not torch.cuda.is_available():
        sys.exit("raw_time.py needs a HIP GPU")
    L = args.samples
    banks = {
        "integer": dict(decim=ct.DECIM, taps=stream.lowpass_taps(ct.NTAPS, 0.5 / ct.DECIM), period=ct.PERIOD,
                        steps=ct.STEPS),
        "rational": dict(decim=rt.DECIM, taps=stream.lowpass_taps(rt.NTAPS, 0.5 / rt.DECIM, gain=rt.INTERP),
                         period=rt.PERIOD, steps=rt.STEPS, interp=rt.INTERP),
    }
    formats = {"cs16": (torch.int16, -32768, 32768), "cs8": (torch.int8, -128, 128), "cu8": (torch.uint8, 0, 256)}

    def window(fn, calls):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(calls):
            fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) / calls

    def alternate(fns):
        for fn in fns.values():
            window(fn, 2)
        t = {k: [] for k in fns}
        for _ in range(args.repeats):
            for k, fn in fns.items():
                t[k].append(window(fn, args.calls))
        return {k + "_ms": spread(v) for k, v in t.items()}

    row = {"device": torch.cuda.get_device_name(0), "samples": L, "windows": args.repeats,
           "calls_per_window": args.calls}
    g = torch.Generator(device="cuda").manual_seed(1)
    for name, kw in banks.items():
        chan = stream.Channelizer(**kw)
        W = chan.outputs(L)
        out = torch.empty((chan.channels, W), dtype=torch.complex64, device="cuda")
        bank = {"channels": chan.channels, "ntaps": chan.ntaps, "interp": chan.interp, "decim": chan.decim,
                "period": chan.period, "outputs_per_channel": W}
        for fmt, (dtype, lo, hi) in formats.items():
            raw = torch.randint(lo, hi, (L, 2), generator=g, device="cuda", dtype=dtype)
            x = stream.raw_to_complex(raw)
            want = chan.run(x).view(torch.int64)
            assert torch.equal(chan.run(raw, out=out).view(torch.int64), want), (name, fmt)
            del want

            def f_raw():
                chan.run(raw, out=out)

            def f_convert():
                chan.run(stream.raw_to_complex(raw), out=out)

            def f_float():
                chan.run(x, out=out)

            r = alternate({"raw": f_raw, "convert_then_float": f_convert, "float": f_float})
            a, b = r["raw_ms"], r["convert_then_float_ms"]
            r["raw_below_convert_then_float"] = b["median"] - a["median"] > b["max"] - b["min"]
            r["convert_then_float_over_raw"] = b["median"] / a["median"]
            r["raw_over_float"] = a["median"] / r["float_ms"]["median"]
            r["input_bytes"] = {"raw": raw.numel() * raw.element_size(), "complex64": x.numel() * 8}
            bank[fmt] = r
            print(json.dumps({name: {fmt: r}}), flush=True)
            del raw, x
            torch.cuda.empty_cache()
        row[name] = bank
        del out

    # (d) host-to-device copies from pinned memory
    copies = {}
    for fmt, (dtype, lo, hi) in formats.items():
        h_raw = torch.randint(lo, hi, (L, 2), dtype=dtype).pin_memory()
        h_x = stream.raw_to_complex(h_raw).pin_memory()
        d_raw, d_x = torch.empty_like(h_raw, device="cuda"), torch.empty_like(h_x, device="cuda")
        r = alternate({"raw": lambda: d_raw.copy_(h_raw, non_blocking=True),
                       "complex64": lambda: d_x.copy_(h_x, non_blocking=True)})
        r["bytes"] = {"raw": h_raw.numel() * h_raw.element_size(), "complex64": h_x.numel() * 8}
        r["complex64_over_raw"] = r["complex64_ms"]["median"] / r["raw_ms"]["median"]
        copies[fmt] = r
        print(json.dumps({"h2d_copy": {fmt: r}}), flush=True)
        del h_raw, h_x, d_raw, d_x
    row["h2d_copy_pinned"] = copies
    for item in args.attach:
        key, path = item.split("=", 1)
        with open(path) as fh:
            row[key] = json.load(fh)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(row, fh, indent=1)


if __name__ == "__main__":
    main()
