"""Time the sliding detector scan (DemodPlan.scan) beside the same work done the only way it
could be done before: the overlapping windows materialised (``x.unfold(0, step, hop)`` copied
into a [W, step] tensor) and given to DemodPlan.detect_metrics.  One stream of 2^24 samples at
SF7 and at SF12, hop = step // 4, a RAW plan with dechirp (what the frame finder scans with).
A one-off measurement for DESIGN.md, not part of bench.py.  Needs a HIP GPU.

Per shape, in milliseconds per call, each the median (with the range) over ``--repeats``
device-event windows of back-to-back calls on one stream after warm-up, the three alternating
in the same process so a drift of the machine shows in all of them:
  scan            plan.scan(x, hop) into pre-allocated outputs
  copy_metrics    the copy of the windows into a pre-allocated [W, step] tensor, then
                  detect_metrics on it (outputs pre-allocated)
  metrics_only    detect_metrics on the windows already materialised (the copy excluded)
The outputs of the two paths are compared bit for bit before anything is timed.

usage: python tools/scan_time.py [--repeats 5] [--samples 16777216] [--out file.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lora-sdr-lightweight-standalone-library-_amd"))

# (sf, calls per window)
SHAPES = ((7, 10), (12, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--samples", type=int, default=1 << 24)
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch

    import lora_phy_amd as amd

    if not torch.cuda.is_available():
        sys.exit("scan_time.py needs a HIP GPU")
    rows = []
    for sf, calls in SHAPES:
        step = 1 << sf
        hop = step // 4
        frame = 66 * step
        F = -(-args.samples // frame)
        g = torch.Generator(device="cpu").manual_seed(sf)
        syms = torch.randint(0, 1 << sf, (F, 64), generator=g, dtype=torch.int32)
        x = amd.modulate(syms.cuda(), sf, 1, 125000, 1.0, 0x12).reshape(-1)[:args.samples].clone()
        x += 0.1 * torch.randn(x.shape[0], dtype=torch.complex64, device="cuda")
        plan = amd.DemodPlan(sf, dechirp=True, mode="raw")
        W = plan.scan_windows(x.shape[0], hop)
        met = plan.scan(x, hop)
        wins = torch.empty((W, step), dtype=torch.complex64, device="cuda")
        wins.copy_(x.unfold(0, step, hop))
        ref = plan.detect_metrics(wins)
        torch.cuda.synchronize()
        for k in ("power", "power_avg", "f_index"):
            a, b = getattr(met, k).reshape(-1), getattr(ref, k).reshape(-1)
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), k
        assert torch.equal(met.index.reshape(-1).to(torch.int32), ref.index.reshape(-1).to(torch.int32))

        def window(fn, n):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(n):
                fn()
            t1.record()
            t1.synchronize()
            return t0.elapsed_time(t1) / n

        def f_scan():
            plan.scan(x, hop, out=met)

        def f_copy():
            wins.copy_(x.unfold(0, step, hop))
            plan.detect_metrics(wins, out=ref)

        def f_only():
            plan.detect_metrics(wins, out=ref)

        fns = {"scan": f_scan, "copy_metrics": f_copy, "metrics_only": f_only}
        for fn in fns.values():
            window(fn, 2)
        t = {k: [] for k in fns}
        for _ in range(args.repeats):
            for k, fn in fns.items():
                t[k].append(window(fn, calls))
        row = {"sf": sf, "samples": x.shape[0], "hop": hop, "windows": W, "calls_per_window": calls}
        for k, v in t.items():
            row[k + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
        row["scan_Mwindows_per_s"] = W / row["scan_ms"]["median"] / 1e3
        row["scan_over_copy_metrics"] = row["scan_ms"]["median"] / row["copy_metrics_ms"]["median"]
        row["scan_over_metrics_only"] = row["scan_ms"]["median"] / row["metrics_only_ms"]["median"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del x, wins, met, ref, plan
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "windows": args.repeats, "shapes": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
