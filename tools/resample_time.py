"""Time the rational-rate down-converter bank (stream.Channelizer.run with interp > 1) beside
the integer bank on the same input and beside the torch formulation a user would write without
it.  One stream of 32 Mi wideband samples of noise into 8 channels, interp 5, decim 96, 385
taps, period 12 - a 2.4 MS/s capture with 200 kHz channel spacing brought to 125 kS/s - on one
GPU, in one process, with the same input.  A one-off measurement for DESIGN.md, not part of
bench.py.  Needs a HIP GPU.

Each figure is the median (with the range) over ``--repeats`` device-event windows of
back-to-back calls on one stream after warm-up, the three alternating so a drift of the machine
shows in all:
  resample      Channelizer(96, taps, 12, steps, interp=5).run(x, out=...) into a pre-allocated
                [C, W] tensor: one kernel that reads x once
  integer       Channelizer(19, 77 taps, 12, steps).run(x, out=...): the integer bank on the same
                input bytes with about the same taps per output (77 against 385 / 5) - a
                different filter and rate, timed as a yardstick only
  torch         for each channel: x * osc[c] (the oscillator pre-computed and resident, its
                generation not timed), view_as_real, then for each of the 5 residues a conv1d of
                that residue's sub-filter at stride 96 (groups=2), written into out[c, r::5]: one
                pass over the wideband data per channel and five strided ones over the product
The bytes a bank has to move are the input once and its outputs once; the fraction of the 8 TB/s
HBM peak is those bytes over the median time.  The resample and torch results are compared (to
1e-4 of the largest output: torch's convolution sums in another order and may contract) before
anything is timed.

usage: python tools/resample_time.py [--repeats 5] [--samples 33554432] [--out file.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lora-sdr-lightweight-standalone-library-_amd"))

HBM_PEAK = 8.0e12  # bytes per second, the MI355X data-sheet figure
CHANNELS, NTAPS, INTERP, DECIM, PERIOD = 8, 385, 5, 96, 12
STEPS = (-4, -3, -2, -1, 0, 1, 2, 3)
INT_NTAPS, INT_DECIM = 77, 19


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--samples", type=int, default=1 << 25)
    ap.add_argument("--calls", type=int, default=5, help="bank calls per timed window")
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch
    import torch.nn.functional as F

    from lora_phy_amd import stream

    if not torch.cuda.is_available():
        sys.exit("resample_time.py needs a HIP GPU")
    L = args.samples
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.view_as_complex(torch.randn((L, 2), generator=g, device="cuda", dtype=torch.float32))
    chan = stream.Channelizer(DECIM, stream.lowpass_taps(NTAPS, 0.5 / DECIM, gain=INTERP), PERIOD, STEPS,
                              interp=INTERP)
    W = chan.outputs(L)
    out = torch.empty((CHANNELS, W), dtype=torch.complex64, device="cuda")
    chan.run(x, out=out)
    ichan = stream.Channelizer(INT_DECIM, stream.lowpass_taps(INT_NTAPS, 0.5 / INT_DECIM), PERIOD, STEPS)
    IW = ichan.outputs(L)
    iout = torch.empty((CHANNELS, IW), dtype=torch.complex64, device="cuda")
    ichan.run(x, out=iout)
    torch.cuda.synchronize()

    # the torch formulation: resident oscillators, each residue's sub-filter as a grouped conv1d
    # weight (conv1d correlates, as the definition does), its outputs interleaved
    n = torch.arange(L, device="cuda", dtype=torch.int64)
    osc = [chan.nco[(n * (k % PERIOD)) % PERIOD] for k in STEPS]
    del n
    res = []
    for r in range(INTERP):
        j0 = (-(r * DECIM)) % INTERP
        off = (r * DECIM + j0) // INTERP
        sub = chan.taps[j0::INTERP]
        res.append((off, (W - 1 - r) // INTERP + 1, sub.reshape(1, 1, -1).repeat(2, 1, 1).contiguous()))
    tout = torch.empty((CHANNELS, 2, W), dtype=torch.float32, device="cuda")

    def f_torch():
        for c in range(CHANNELS):
            z = torch.view_as_real(x * osc[c]).t().unsqueeze(0)  # [1, 2, L]
            for r, (off, nu, weight) in enumerate(res):
                tout[c, :, r::INTERP] = F.conv1d(z[:, :, off:], weight, stride=DECIM, groups=2)[0, :, :nu]

    def f_chan():
        chan.run(x, out=out)

    def f_int():
        ichan.run(x, out=iout)

    f_torch()
    torch.cuda.synchronize()
    scale = float(out.abs().max())
    err = float((torch.complex(tout[:, 0], tout[:, 1]) - out).abs().max())
    assert scale > 0 and err <= 1e-4 * scale, (err, scale)

    def window(fn, calls):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(calls):
            fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) / calls

    fns = {"resample": (f_chan, args.calls), "integer": (f_int, args.calls), "torch": (f_torch, 1)}
    for fn, calls in fns.values():
        window(fn, 2)
    t = {k: [] for k in fns}
    for _ in range(args.repeats):
        for k, (fn, calls) in fns.items():
            t[k].append(window(fn, calls))
    moved = L * 8 + CHANNELS * W * 8
    imoved = L * 8 + CHANNELS * IW * 8
    row = {"device": torch.cuda.get_device_name(0), "samples": L, "channels": CHANNELS, "ntaps": NTAPS,
           "interp": INTERP, "decim": DECIM, "period": PERIOD, "outputs_per_channel": W,
           "integer_ntaps": INT_NTAPS, "integer_decim": INT_DECIM, "integer_outputs_per_channel": IW,
           "windows": args.repeats, "bank_calls_per_window": args.calls, "bytes_moved": moved,
           "integer_bytes_moved": imoved, "torch_max_error_over_largest_output": err / scale}
    for k, v in t.items():
        row[k + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    med, imed = row["resample_ms"]["median"], row["integer_ms"]["median"]
    row["resample_GB_per_s"] = moved / med / 1e6
    row["fraction_of_hbm_peak"] = moved / (med * 1e-3) / HBM_PEAK
    row["integer_GB_per_s"] = imoved / imed / 1e6
    row["integer_fraction_of_hbm_peak"] = imoved / (imed * 1e-3) / HBM_PEAK
    row["resample_over_integer"] = med / imed
    row["torch_over_resample"] = row["torch_ms"]["median"] / med
    print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(row, fh, indent=1)


if __name__ == "__main__":
    main()
