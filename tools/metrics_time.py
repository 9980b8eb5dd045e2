"""Time the per-symbol detector metrics (DemodPlan.detect_metrics) beside the demodulator's own
step (DemodPlan.run) at the project's batch shapes: BASELINE.json configs[1] (SF7) and
configs[2] (SF12), 15,625 frames of 2 + 64 symbols each, generated on the device as bench.py
generates them.  A one-off measurement for DESIGN.md, not part of bench.py.  Needs a HIP GPU.

Per shape, in milliseconds per call: `detect_metrics` with its outputs pre-allocated and
`plan.run` with its outputs pre-allocated, each the median (with the range) over `--repeats`
device-event windows of back-to-back calls on one stream after warm-up, the two alternating
in the same process so a drift of the machine shows in both; and their ratio.  The metrics
kernel adds every symbol's |X|^2 in bin order in one lane (the detector's double total is
order-dependent), so its time grows with N per symbol where the demodulator's does not.

usage: python tools/metrics_time.py [--repeats 5] [--frames 15625] [--out file.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lora-sdr-lightweight-standalone-library-_amd"))

# (sf, data symbols per frame, calls per window of detect_metrics, of plan.run)
SHAPES = ((7, 64, 20, 100), (12, 64, 3, 10))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=15625)
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch

    import lora_phy_amd as amd

    if not torch.cuda.is_available():
        sys.exit("metrics_time.py needs a HIP GPU")
    rows = []
    for sf, data_syms, n_met, n_run in SHAPES:
        g = torch.Generator(device="cpu").manual_seed(sf)
        syms = torch.randint(0, 1 << sf, (args.frames, data_syms), generator=g, dtype=torch.int32)
        iq = amd.modulate(syms.cuda(), sf, 1, 125000, 1.0, 0x12)
        plan = amd.DemodPlan(sf, dechirp=True)
        res = plan.run(iq)
        met = plan.detect_metrics(iq, res)
        torch.cuda.synchronize()
        got = res.symbols.cpu().numpy()
        assert (got == syms.numpy()).all() and (met.index.cpu().numpy()[:, 2:] == got).all()

        def window(fn, n):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(n):
                fn()
            t1.record()
            t1.synchronize()
            return t0.elapsed_time(t1) / n

        def f_met():
            plan.detect_metrics(iq, res, out=met)

        def f_run():
            plan.run(iq, out=res)

        window(f_met, 2)
        window(f_run, n_run)
        tm, tr = [], []
        for _ in range(args.repeats):
            tm.append(window(f_met, n_met))
            tr.append(window(f_run, n_run))
        row = {"sf": sf, "frames": args.frames, "symbols_per_frame": data_syms + 2,
               "detect_metrics_ms": {"median": statistics.median(tm), "min": min(tm), "max": max(tm),
                                     "calls_per_window": n_met},
               "plan_run_ms": {"median": statistics.median(tr), "min": min(tr), "max": max(tr),
                               "calls_per_window": n_run},
               "metrics_over_run": statistics.median(tm) / statistics.median(tr),
               "metrics_Msymbols_per_s": args.frames * (data_syms + 2) / statistics.median(tm) / 1e3}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del iq, res, met, plan
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "windows": args.repeats, "shapes": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
