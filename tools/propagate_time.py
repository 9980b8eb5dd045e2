"""Time the propagation stage (stream.propagate) on one GPU, in one process: 2^25 complex64 samples
as one row and as 32 rows, 1, 2 and 8 paths at 16 taps, with and without the rotation; beside it
``stream.impair`` with a gain and a carrier offset (a pure streaming kernel, for scale) and what
torch can do at all - no clock offset and one phase per path, so that a path is one FIR and the
channel the composed FIR of its paths, a ``conv1d`` per row.  A one-off measurement for DESIGN.md,
not part of bench.py.  Needs a HIP GPU.

Each figure is the median (with the range) over ``--repeats`` device-event windows of
back-to-back calls on one stream after warm-up, the candidates alternating so a drift of the
machine shows in all of them.  Every output is pre-allocated where the candidate allows it, and
``propagate`` is given its parameters as device arrays, so no call builds or copies one.  The
bytes a candidate has to move are its input once and its output once (16 a sample); they are given
over the median time as a fraction of the 8 TB/s HBM peak.

usage: python tools/propagate_time.py [--repeats 5] [--samples 33554432] [--out file.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lora-sdr-lightweight-standalone-library-_amd"))

HBM_PEAK = 8.0e12  # bytes per second, the MI355X data-sheet figure
DELAYS = [0.37, 1.5, -2.25, 7.625, 12.0, 0.996, 30.5, -0.125]
GAINS = [1.0, 0.5j, -0.25, 0.125 + 0.125j, 0.1, -0.1j, 0.05, 0.05j]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--samples", type=int, default=1 << 25)
    ap.add_argument("--calls", type=int, default=5, help="kernel calls per timed window")
    ap.add_argument("--out")
    args = ap.parse_args()

    import numpy as np
    import torch

    from lora_phy_amd import stream

    if not torch.cuda.is_available():
        sys.exit("propagate_time.py needs a HIP GPU")
    total = args.samples
    g = torch.Generator(device="cuda").manual_seed(1)
    flat = torch.view_as_complex(torch.randn((total, 2), generator=g, device="cuda", dtype=torch.float32) * 0.2)
    out_flat = torch.empty(total, dtype=torch.complex64, device="cuda")
    table = torch.from_numpy(stream.fracdelay_table()).cuda()
    table_np = stream.fracdelay_table().astype(np.float64)
    fns = {}
    for R in (1, 32):
        x, out = flat.view(R, total // R), out_flat.view(R, total // R)
        for P in (1, 2, 8):
            d = torch.tensor([[stream.delay_word(v) for v in DELAYS[:P]]] * R, dtype=torch.int64, device="cuda")
            gn = torch.tensor([GAINS[:P]] * R, dtype=torch.complex64, device="cuda")
            sfo = torch.full((R,), stream.sfo_word(20.0), dtype=torch.int64, device="cuda")
            rot = dict(cfo=torch.full((R,), stream.cfo_word64(0.25 / 128), dtype=torch.int64, device="cuda"),
                       drift=torch.full((R,), stream.drift_word(100.0, 125e3), dtype=torch.int64, device="cuda"))
            base = dict(delay=d, gain=gn, sfo_ppm=sfo, table=table, out=out)
            fns[f"propagate_r{R}_p{P}"] = (lambda x=x, kw=base: stream.propagate(x, **kw), args.calls)
            fns[f"propagate_r{R}_p{P}_rot"] = (lambda x=x, kw=dict(base, **rot): stream.propagate(x, **kw), args.calls)
            # torch: the composed FIR of the paths (sfo = 0), one complex conv1d as four real ones
            # a path reads x[n + q - 7 + t] through table[ph][t]: as a filter, lag -q + 7 - t
            terms = []
            for v, a in zip(DELAYS[:P], GAINS[:P]):
                w = stream.delay_word(v)
                q, ph = (-w) >> 32, ((-w) & 0xFFFFFFFF) >> 24
                terms += [(-q + 7 - t, a * table_np[ph, t]) for t in range(16)]
            lo = min(lag for lag, _ in terms)
            span = max(lag for lag, _ in terms) - lo + 1
            h = np.zeros(span, np.complex128)
            for lag, c in terms:
                h[lag - lo] += c
            k = torch.from_numpy(h[::-1].copy()).to(torch.complex64).cuda()   # conv1d correlates
            wr, wi = k.real.reshape(1, 1, -1).contiguous(), k.imag.reshape(1, 1, -1).contiguous()

            def f_conv(x=x, wr=wr, wi=wi, span=span):
                xr = torch.view_as_real(x)
                a, b = xr[..., 0].unsqueeze(1), xr[..., 1].unsqueeze(1)
                c = torch.nn.functional.conv1d
                pad = span - 1
                re = c(a, wr, padding=pad) - c(b, wi, padding=pad)
                im = c(a, wi, padding=pad) + c(b, wr, padding=pad)
                return torch.complex(re, im)

            fns[f"torch_conv1d_r{R}_p{P}"] = (f_conv, 1)
        gain = torch.full((R,), 0.5, dtype=torch.float32, device="cuda")
        fcw = torch.full((R,), stream.cfo_word(0.25 / 128), dtype=torch.int32, device="cuda")
        fns[f"impair_gain_cfo_r{R}"] = (lambda x=x, out=out, gain=gain, fcw=fcw:
                                        stream.impair(x, gain=gain, cfo=fcw, out=out), args.calls)

    def window(fn, calls):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(calls):
            fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) / calls

    for fn, calls in fns.values():
        window(fn, 2)
    t = {k: [] for k in fns}
    for _ in range(args.repeats):
        for k, (fn, calls) in fns.items():
            t[k].append(window(fn, calls))
    row = {"device": torch.cuda.get_device_name(0), "samples": total, "taps": 16, "sfo_ppm": 20.0,
           "delays_samples": DELAYS, "windows": args.repeats, "kernel_calls_per_window": args.calls}
    for k, v in t.items():
        med = statistics.median(v)
        nbytes = 16 * total
        row[k] = {"ms": {"median": med, "min": min(v), "max": max(v)}, "bytes_moved": nbytes,
                  "GB_per_s": nbytes / (med * 1e-3) / 1e9, "fraction_of_hbm_peak": nbytes / (med * 1e-3) / HBM_PEAK,
                  "Gsamples_per_s": total / (med * 1e-3) / 1e9}
    print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(row, fh, indent=1)


if __name__ == "__main__":
    main()
