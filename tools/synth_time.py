"""Time the synthesis bank (stream.Synthesizer.run) beside what a user would write without it.
8 channels of 4 Mi samples into one stream of 32 Mi wideband samples, 65 taps, interp 8, on one
GPU, in one process, with the same inputs.  A one-off measurement for DESIGN.md, not part of
bench.py.  Needs a HIP GPU.

Each figure is the median (with the range) over ``--repeats`` device-event windows of
back-to-back calls on one stream after warm-up, the candidates alternating so a drift of the
machine shows in all of them.  Every output is pre-allocated where the candidate allows it.
  synth_cf32 / synth_cs16 / synth_cs8
                Synthesizer.run(chans, out=..., dtype=...): one kernel that reads the channel
                streams once and writes each wideband sample once, in that format
  torch         baseline 1 - per channel: view_as_real, conv_transpose1d(groups=2, stride=interp)
                with the taps, the "valid" slice, a multiply by that channel's oscillator (pre-
                computed and resident, its generation not timed) and the sum over the channels
  synth_then_quantize_cs16 / _cs8
                baseline 2 - the complex64 kernel followed by iq_io.quantize: the passes over a
                complex64 copy that the raw store removes
The bytes the kernel has to move are the inputs once and the output once; the output bytes over
the median time are given as a fraction of the 8 TB/s HBM peak.  The torch result is compared
with the kernel's (to a tolerance: torch's convolution sums in another order and may contract),
and baseline 2's codes with the raw kernel's (equal at these power-of-two scales), before anything
is timed.

usage: python tools/synth_time.py [--repeats 5] [--samples 4194304] [--out file.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lora-sdr-lightweight-standalone-library-_amd"))

HBM_PEAK = 8.0e12  # bytes per second, the MI355X data-sheet figure
CHANNELS, NTAPS, INTERP, PERIOD = 8, 65, 8, 16
STEPS = (-7, -5, -3, -1, 1, 3, 5, 7)
GAIN = 0.1  # keeps the sum of the channels inside the raw formats' range


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--samples", type=int, default=1 << 22, help="samples per channel")
    ap.add_argument("--calls", type=int, default=5, help="kernel calls per timed window")
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch
    import torch.nn.functional as F

    from lora_phy_amd import iq_io, stream

    if not torch.cuda.is_available():
        sys.exit("synth_time.py needs a HIP GPU")
    Lc = args.samples
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.view_as_complex(torch.randn((CHANNELS, Lc, 2), generator=g, device="cuda", dtype=torch.float32))
    taps = stream.lowpass_taps(NTAPS, 0.5 / INTERP, gain=INTERP)
    syn = stream.Synthesizer(INTERP, taps, PERIOD, STEPS, [GAIN] * CHANNELS)
    W, P = syn.outputs(Lc), syn.P
    outs = {None: torch.empty(W, dtype=torch.complex64, device="cuda"),
            torch.int16: torch.empty((W, 2), dtype=torch.int16, device="cuda"),
            torch.int8: torch.empty((W, 2), dtype=torch.int8, device="cuda")}
    for dt, o in outs.items():
        syn.run(x, out=o, dtype=dt)
    torch.cuda.synchronize()

    # baseline 1: resident oscillators, the taps as a grouped conv_transpose1d weight
    n = torch.arange(W, device="cuda", dtype=torch.int64)
    osc = [syn.nco[(n * (k % PERIOD)) % PERIOD] for k in STEPS]
    del n
    weight = (GAIN * syn.taps).reshape(1, 1, NTAPS).repeat(2, 1, 1).contiguous()
    lo = (P - 1) * INTERP

    def f_torch():
        y = None
        for c in range(CHANNELS):
            z = torch.view_as_real(x[c]).t().unsqueeze(0)                   # [1, 2, Lc]
            s = F.conv_transpose1d(z, weight, stride=INTERP, groups=2)[0, :, lo:lo + W]
            s = torch.complex(s[0], s[1]) * osc[c]
            y = s if y is None else y.add_(s)
        return y

    def f_quantize(dt):
        return lambda: iq_io.quantize(syn.run(x, out=outs[None]), dt)

    ref = f_torch()
    torch.cuda.synchronize()
    scale = float(outs[None].abs().max())
    err = float((ref - outs[None]).abs().max())
    assert err <= 1e-4 * scale, (err, scale)
    del ref
    for dt in (torch.int16, torch.int8):
        assert torch.equal(f_quantize(dt)(), outs[dt]), dt
    peak = float(torch.view_as_real(outs[None]).abs().max())

    def window(fn, calls):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(calls):
            fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) / calls

    fns = {"synth_cf32": (lambda: syn.run(x, out=outs[None]), args.calls),
           "synth_cs16": (lambda: syn.run(x, out=outs[torch.int16], dtype=torch.int16), args.calls),
           "synth_cs8": (lambda: syn.run(x, out=outs[torch.int8], dtype=torch.int8), args.calls),
           "torch": (f_torch, 1),
           "synth_then_quantize_cs16": (f_quantize(torch.int16), 1),
           "synth_then_quantize_cs8": (f_quantize(torch.int8), 1)}
    for fn, calls in fns.values():
        window(fn, 2)
    t = {k: [] for k in fns}
    for _ in range(args.repeats):
        for k, (fn, calls) in fns.items():
            t[k].append(window(fn, calls))
    row = {"device": torch.cuda.get_device_name(0), "channels": CHANNELS, "samples_per_channel": Lc,
           "ntaps": NTAPS, "interp": INTERP, "period": PERIOD, "gain": GAIN, "outputs": W,
           "peak_output_component": peak, "windows": args.repeats, "kernel_calls_per_window": args.calls,
           "bytes_read": CHANNELS * Lc * 8}
    for k, v in t.items():
        row[k + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    for k, sb in (("synth_cf32", 8), ("synth_cs16", 4), ("synth_cs8", 2)):
        med = row[k + "_ms"]["median"] * 1e-3
        row[k + "_bytes_written"] = W * sb
        row[k + "_write_GB_per_s"] = W * sb / med / 1e9
        row[k + "_write_fraction_of_hbm_peak"] = W * sb / med / HBM_PEAK
        row[k + "_Gsamples_per_s"] = W / med / 1e9
    row["torch_over_synth_cf32"] = row["torch_ms"]["median"] / row["synth_cf32_ms"]["median"]
    for f in ("cs16", "cs8"):
        row["synth_then_quantize_over_synth_" + f] = (row["synth_then_quantize_%s_ms" % f]["median"] /
                                                      row["synth_%s_ms" % f]["median"])
    print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(row, fh, indent=1)


if __name__ == "__main__":
    main()
