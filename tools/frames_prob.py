"""Measure what stream.receive_frames_device returns from noisy streams of self-describing
frames of mixed lengths (awgn.sweep_receive_frames): the share of planted frames returned at
their exact start with status OK and the exact payload, and the false frames per 10^6 windows -
at thresh_db = 0 and at one negative threshold per SF, which the header gate is there to make
usable.  SF 7, 9 and 12 at osr 1, hop = step / 4, payloads of 0 .. 16 bytes at rate 4/5 with the
CRC.  A one-off measurement for DESIGN.md, not a gate and not part of bench.py.  Needs a HIP GPU.

The negative threshold is chosen from noise-only rows, per SF: ``--grid`` thresholds are tried
on at least ``--pick-windows`` windows of noise alone, and the lowest one is taken at which noise
lists at most half the candidates the default candidate capacity holds (one slot per four
symbols of the row) - below that, noise alone would crowd real frames out of the list.  The
candidates per window at every tried threshold are recorded with the choice.

usage: python tools/frames_prob.py [--frames 1000] [--noise-windows 2000000] [--out file.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lora-sdr-lightweight-standalone-library-_amd"))

SFS = (7, 9, 12)
SNRS = list(range(-16, 7, 2))
MAX_BYTES, CR = 16, 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--noise-windows", type=int, default=2_000_000)
    ap.add_argument("--pick-windows", type=int, default=200_000)
    ap.add_argument("--grid", type=float, nargs="*", default=[-2.0, -4.0, -6.0, -8.0, -10.0, -12.0, -14.0])
    ap.add_argument("--sf", type=int, nargs="*", default=list(SFS))
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch

    from lora_phy_amd import awgn

    if not torch.cuda.is_available():
        sys.exit("frames_prob.py needs a HIP GPU")
    row = {"device": torch.cuda.get_device_name(0), "osr": 1, "hop": "step / 4", "max_bytes": MAX_BYTES, "rdd": CR,
           "frames_per_point": args.frames, "snr_db": SNRS, "threshold_choice": [], "sweeps": [], "noise_only": []}
    for sf in args.sf:
        # the negative threshold, from noise alone
        tried, chosen = [], 0.0
        for th in sorted(args.grid, reverse=True):
            rec = awgn.sweep_receive_frames(sf, [], max_bytes=MAX_BYTES, cr=CR, thresh_db=th, seed=2026 + sf,
                                            noise_windows=args.pick_windows)[-1]
            tried.append({"thresh_db": th, "candidates_per_window": rec["candidates_per_window"],
                          "capacity_per_window": rec["candidate_capacity_per_window"],
                          "false_frames": rec["false_frames"], "windows": rec["windows"]})
            if rec["candidates_per_window"] > 0.5 * rec["candidate_capacity_per_window"]:
                break
            chosen = th
        row["threshold_choice"].append({"sf": sf, "chosen_thresh_db": chosen, "tried": tried})
        print(json.dumps(row["threshold_choice"][-1]), flush=True)
        for th in sorted({0.0, chosen}, reverse=True):
            t0 = time.time()
            recs = awgn.sweep_receive_frames(sf, SNRS, frames=args.frames, max_bytes=MAX_BYTES, cr=CR, thresh_db=th,
                                             seed=2026 + sf, noise_windows=args.noise_windows)
            row["noise_only"].append(recs.pop())
            keys = ("returned_ok", "found_at_planted", "false_frames", "false_frames_ok", "candidates",
                    "candidates_dropped", "p_ok", "false_frames_per_million_windows")
            row["sweeps"].append({"sf": sf, "thresh_db": th, "planted": recs[0]["planted"],
                                  "windows": recs[0]["windows"], "max_symbols": recs[0]["max_symbols"],
                                  **{k: [r[k] for r in recs] for k in keys}, "seconds": time.time() - t0})
            print(json.dumps(row["sweeps"][-1]), flush=True)
    print(json.dumps(row["noise_only"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(row, fh, indent=1)


if __name__ == "__main__":
    main()
