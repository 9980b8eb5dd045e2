"""Time the down-converter bank (stream.Channelizer.run) beside the torch formulation a user
would write without it: per channel, a multiply of the wideband stream by that channel's
oscillator, then ``conv1d`` with the taps at stride ``decim`` on the real and imaginary parts.
One stream of 32 Mi wideband samples into 8 channels, 65 taps, decim 8, on one GPU, in one
process, with the same inputs.  A one-off measurement for DESIGN.md, not part of bench.py.
Needs a HIP GPU.

Each figure is the median (with the range) over ``--repeats`` device-event windows of
back-to-back calls on one stream after warm-up, the two alternating so a drift of the machine
shows in both:
  channelizer   Channelizer.run(x, out=...) into a pre-allocated [C, W] tensor: one kernel that
                reads x once
  torch         for each channel: x * osc[c] (the oscillator pre-computed and resident, its
                generation not timed), view_as_real, conv1d(groups=2, stride=decim): one pass over
                the wideband data per channel, into pre-allocated outputs where torch allows
The bytes the channelizer has to move are the input once and the outputs once; the fraction of
the 8 TB/s HBM peak is those bytes over the median time.  The two results are compared (to a
tolerance: torch's convolution sums in another order and may contract) before anything is timed.

usage: python tools/channel_time.py [--repeats 5] [--samples 33554432] [--out file.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lora-sdr-lightweight-standalone-library-_amd"))

HBM_PEAK = 8.0e12  # bytes per second, the MI355X data-sheet figure
CHANNELS, NTAPS, DECIM, PERIOD = 8, 65, 8, 16
STEPS = (-7, -5, -3, -1, 1, 3, 5, 7)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--samples", type=int, default=1 << 25)
    ap.add_argument("--calls", type=int, default=5, help="channelizer calls per timed window")
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch
    import torch.nn.functional as F

    from lora_phy_amd import stream

    if not torch.cuda.is_available():
        sys.exit("channel_time.py needs a HIP GPU")
    L = args.samples
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.view_as_complex(torch.randn((L, 2), generator=g, device="cuda", dtype=torch.float32))
    taps = stream.lowpass_taps(NTAPS, 0.5 / DECIM)
    chan = stream.Channelizer(DECIM, taps, PERIOD, STEPS)
    W = chan.outputs(L)
    out = torch.empty((CHANNELS, W), dtype=torch.complex64, device="cuda")
    chan.run(x, out=out)
    torch.cuda.synchronize()

    # the torch formulation: resident oscillators, the taps as a grouped conv1d weight
    n = torch.arange(L, device="cuda", dtype=torch.int64)
    osc = [chan.nco[(n * (k % PERIOD)) % PERIOD] for k in STEPS]
    del n
    weight = chan.taps.flip(0).reshape(1, 1, NTAPS).repeat(2, 1, 1).contiguous()  # conv1d correlates

    def torch_channel(c):
        z = torch.view_as_real(x * osc[c]).t().unsqueeze(0)  # [1, 2, L]
        return F.conv1d(z, weight, stride=DECIM, groups=2)   # [1, 2, W]

    def f_torch():
        return [torch_channel(c) for c in range(CHANNELS)]

    def f_chan():
        chan.run(x, out=out)

    ref = f_torch()
    torch.cuda.synchronize()
    scale = float(out.abs().max())
    for c in range(CHANNELS):
        y = torch.complex(ref[c][0, 0], ref[c][0, 1])
        # the taps are symmetric, so the flip changes nothing but the order of the sum
        err = float((y - out[c]).abs().max())
        assert err <= 1e-4 * scale, (c, err, scale)
    del ref, y

    def window(fn, calls):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(calls):
            fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) / calls

    fns = {"channelizer": (f_chan, args.calls), "torch": (f_torch, 1)}
    for fn, calls in fns.values():
        window(fn, 2)
    t = {k: [] for k in fns}
    for _ in range(args.repeats):
        for k, (fn, calls) in fns.items():
            t[k].append(window(fn, calls))
    moved = L * 8 + CHANNELS * W * 8
    row = {"device": torch.cuda.get_device_name(0), "samples": L, "channels": CHANNELS, "ntaps": NTAPS,
           "decim": DECIM, "period": PERIOD, "outputs_per_channel": W, "windows": args.repeats,
           "channelizer_calls_per_window": args.calls, "bytes_moved": moved}
    for k, v in t.items():
        row[k + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    med = row["channelizer_ms"]["median"]
    row["channelizer_GB_per_s"] = moved / med / 1e6
    row["fraction_of_hbm_peak"] = moved / (med * 1e-3) / HBM_PEAK
    row["torch_over_channelizer"] = row["torch_ms"]["median"] / med
    print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(row, fh, indent=1)


if __name__ == "__main__":
    main()
