"""Time the channel impairment stage (stream.impair) beside what a user would write without it:
one row of 2^25 complex64 samples with a carrier offset and white Gaussian noise, on one GPU, in
one process, with the same input.  A one-off measurement for DESIGN.md, not part of bench.py.
Needs a HIP GPU.

Each figure is the median (with the range) over ``--repeats`` device-event windows of
back-to-back calls on one stream after warm-up, the candidates alternating so a drift of the
machine shows in all of them.  Every output is pre-allocated where the candidate allows it.
  impair_cf32 / impair_inplace / impair_cs16 / impair_cu8
                impair(x, sigma, cfo, out=...): one kernel that reads the row once and writes it
                once - out of place, in place, and stored as cs16 and cu8 codes
  impair_noise_only
                impair(None, sigma, out=...): nothing read
  impair_rotate_only
                impair(x, cfo, out=...): the noise stage off
  torch_resident_rot
                baseline 1 - ``x * rot + randn * sigma`` with ``rot`` resident (its generation not
                timed): a product pass, an RNG pass, a scale pass and a sum pass
  torch_polar   the same with ``rot = torch.polar(ones, 2 pi cfo n)`` timed (float32 phase)
  torch_then_quantize_cs16
                baseline 1 followed by iq_io.quantize
The bytes a candidate has to move are its input once and its output once; they are given over the
median time as a fraction of the 8 TB/s HBM peak.  Nothing is compared for equality: torch's
generator is another one, which is the point of the stage.

usage: python tools/impair_time.py [--repeats 5] [--samples 33554432] [--out file.json]
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lora-sdr-lightweight-standalone-library-_amd"))

HBM_PEAK = 8.0e12  # bytes per second, the MI355X data-sheet figure
SNR_DB, CFO = 5.0, 0.25 / 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--samples", type=int, default=1 << 25)
    ap.add_argument("--calls", type=int, default=5, help="kernel calls per timed window")
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch

    from lora_phy_amd import iq_io, stream

    if not torch.cuda.is_available():
        sys.exit("impair_time.py needs a HIP GPU")
    L = args.samples
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.view_as_complex(torch.randn((L, 2), generator=g, device="cuda", dtype=torch.float32) * 0.2)
    sigma_f = stream.noise_sigma(SNR_DB, 0.2)
    sigma = torch.full((1,), sigma_f, dtype=torch.float32, device="cuda")
    fcw = torch.full((1,), stream.cfo_word(CFO), dtype=torch.int32, device="cuda")
    out = torch.empty(L, dtype=torch.complex64, device="cuda")
    work = x.clone()
    o16 = torch.empty((L, 2), dtype=torch.int16, device="cuda")
    o8 = torch.empty((L, 2), dtype=torch.uint8, device="cuda")
    n = torch.arange(L, device="cuda", dtype=torch.float32)
    rot = torch.polar(torch.ones(L, device="cuda"), (2.0 * math.pi * CFO) * n)
    noise = torch.empty((L, 2), dtype=torch.float32, device="cuda")

    def f_torch():
        noise.normal_(generator=g)
        return x * rot + torch.view_as_complex(noise * sigma_f)

    def f_polar():
        r = torch.polar(torch.ones_like(n), (2.0 * math.pi * CFO) * n)
        noise.normal_(generator=g)
        return x * r + torch.view_as_complex(noise * sigma_f)

    fns = {"impair_cf32": (lambda: stream.impair(x, sigma=sigma, cfo=fcw, seed=1, out=out), args.calls, 16),
           "impair_inplace": (lambda: stream.impair(work, sigma=sigma, cfo=fcw, seed=1, out=work), args.calls, 16),
           "impair_cs16": (lambda: stream.impair(x, sigma=sigma, cfo=fcw, seed=1, out=o16, dtype=torch.int16),
                           args.calls, 12),
           "impair_cu8": (lambda: stream.impair(x, sigma=sigma, cfo=fcw, seed=1, out=o8, dtype=torch.uint8),
                          args.calls, 10),
           "impair_noise_only": (lambda: stream.impair(None, sigma=sigma, seed=1, out=out, length=L), args.calls, 8),
           "impair_rotate_only": (lambda: stream.impair(x, cfo=fcw, out=out), args.calls, 16),
           "torch_resident_rot": (f_torch, 1, 16),
           "torch_polar": (f_polar, 1, 16),
           "torch_then_quantize_cs16": (lambda: iq_io.quantize(f_torch(), torch.int16), 1, 12)}

    def window(fn, calls):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(calls):
            fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) / calls

    for fn, calls, _ in fns.values():
        window(fn, 2)
    t = {k: [] for k in fns}
    for _ in range(args.repeats):
        for k, (fn, calls, _) in fns.items():
            t[k].append(window(fn, calls))
    row = {"device": torch.cuda.get_device_name(0), "samples": L, "snr_db": SNR_DB, "cfo_cycles_per_sample": CFO,
           "windows": args.repeats, "kernel_calls_per_window": args.calls}
    for k, v in t.items():
        med = statistics.median(v)
        nbytes = fns[k][2] * L
        row[k] = {"ms": {"median": med, "min": min(v), "max": max(v)}, "bytes_moved": nbytes,
                  "GB_per_s": nbytes / (med * 1e-3) / 1e9, "fraction_of_hbm_peak": nbytes / (med * 1e-3) / HBM_PEAK,
                  "Gsamples_per_s": L / (med * 1e-3) / 1e9}
    row["torch_resident_rot_over_impair_cf32"] = (row["torch_resident_rot"]["ms"]["median"] /
                                                  row["impair_cf32"]["ms"]["median"])
    row["impair_cf32_range_below_torch_resident_rot_range"] = (row["impair_cf32"]["ms"]["max"] <
                                                               row["torch_resident_rot"]["ms"]["min"])
    print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(row, fh, indent=1)


if __name__ == "__main__":
    main()
