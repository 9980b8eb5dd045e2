"""Measure what stream.receive_preamble_frames_device returns from noisy streams of preambled
self-describing frames (awgn.sweep_receive_preamble) beside what stream.receive_frames_device
returns for the same payloads sent without a preamble (awgn.sweep_receive_frames), with no carrier
offset and with 3.25 bins of it: the share of planted frames returned at their exact start with
status OK and the exact payload, the false frames, and the candidates dropped.  SF 7, 9 and 12 at
osr 1, hop = step / 4, payloads of 0 .. 16 bytes at rate 4/5 with the CRC, -20 .. +6 dB.  A one-off
measurement for DESIGN.md, not a gate and not part of bench.py.  Needs a HIP GPU.

The preamble finder's two thresholds (one value for both) are chosen from noise-only rows, per
SF, as tools/frames_prob.py chooses its one: ``--grid`` values are tried on at least
``--pick-windows`` windows of noise alone, and the lowest is taken at which noise lists at most
half the candidates the default candidate capacity holds.  The plain chain runs at
``--plain-thresh`` (-14 dB, its own measured choice).  The preambled chain is swept three times:
at the chosen thresholds, the same with four times the candidate capacity, and 6 dB higher.

usage: python tools/preamble_prob.py [--frames 600] [--out file.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lora-sdr-lightweight-standalone-library-_amd"))

SFS = (7, 9, 12)
SNRS = list(range(-20, 7, 2))
MAX_BYTES, CR = 16, 1
KEYS = ("returned_ok", "found_at_planted", "false_frames", "false_frames_ok", "candidates", "candidates_dropped",
        "p_ok", "false_frames_per_million_windows")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--pick-windows", type=int, default=100_000)
    ap.add_argument("--noise-windows", type=int, default=100_000)
    ap.add_argument("--grid", type=float, nargs="*", default=[float(-2 * i) for i in range(0, 15)])
    ap.add_argument("--plain-thresh", type=float, default=-14.0)
    ap.add_argument("--cfo", type=float, nargs="*", default=[0.0, 3.25])
    ap.add_argument("--sf", type=int, nargs="*", default=list(SFS))
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch

    from lora_phy_amd import awgn

    if not torch.cuda.is_available():
        sys.exit("preamble_prob.py needs a HIP GPU")
    row = {"device": torch.cuda.get_device_name(0), "osr": 1, "hop": "step / 4", "max_bytes": MAX_BYTES, "rdd": CR,
           "frames_per_point": args.frames, "snr_db": SNRS, "preamble": 8, "preamble_acc": 6,
           "plain_thresh_db": args.plain_thresh, "threshold_choice": [], "sweeps": [], "noise_only": []}
    for sf in args.sf:
        tried, chosen = [], max(args.grid)
        for th in sorted(args.grid, reverse=True):
            rec = awgn.sweep_receive_preamble(sf, [], max_bytes=MAX_BYTES, cr=CR, thresh_up_db=th, thresh_dn_db=th,
                                              seed=2026 + sf, noise_windows=args.pick_windows)[-1]
            tried.append({"thresh_db": th, "candidates_per_window": rec["candidates_per_window"],
                          "capacity_per_window": rec["candidate_capacity_per_window"],
                          "false_frames": rec["false_frames"], "windows": rec["windows"]})
            if rec["candidates_per_window"] > 0.5 * rec["candidate_capacity_per_window"]:
                break
            chosen = th
        row["threshold_choice"].append({"sf": sf, "chosen_thresh_db": chosen, "tried": tried})
        print(json.dumps(row["threshold_choice"][-1]), flush=True)
        # the preambled chain at the chosen thresholds; the same with four times the candidate
        # capacity (frames lost to a full list come back, frames not found do not); and 6 dB higher
        variants = {"preamble": (chosen, 1), "preamble_cap4": (chosen, 4), "preamble_plus6": (chosen + 6.0, 1)}
        for cfo in args.cfo:
            for chain in ("preamble", "preamble_cap4", "preamble_plus6", "plain"):
                t0 = time.time()
                if chain != "plain":
                    th, mult = variants[chain]
                    recs = awgn.sweep_receive_preamble(sf, SNRS, frames=args.frames, max_bytes=MAX_BYTES, cr=CR,
                                                       thresh_up_db=th, thresh_dn_db=th, cfo_bins=cfo,
                                                       seed=2026 + sf, noise_windows=args.noise_windows,
                                                       cand_capacity_mult=mult)
                else:
                    recs = awgn.sweep_receive_frames(sf, SNRS, frames=args.frames, max_bytes=MAX_BYTES, cr=CR,
                                                     thresh_db=args.plain_thresh, cfo_bins=cfo, seed=2026 + sf,
                                                     noise_windows=args.noise_windows)
                noise = recs.pop()
                noise.update(chain=chain, cfo_bins=cfo)
                row["noise_only"].append(noise)
                sweep = {"sf": sf, "chain": chain, "cfo_bins": cfo,
                         "thresh_db": variants[chain][0] if chain != "plain" else args.plain_thresh,
                         "cand_capacity_mult": variants[chain][1] if chain != "plain" else 1,
                         "planted": recs[0]["planted"], "windows": recs[0]["windows"],
                         "max_symbols": recs[0]["max_symbols"], **{k: [r[k] for r in recs] for k in KEYS},
                         "seconds": time.time() - t0}
                if chain != "plain":
                    sweep["cfo_right"] = [r["cfo_right"] for r in recs]
                row["sweeps"].append(sweep)
                print(json.dumps(sweep), flush=True)
        if args.out:  # (kept after every SF: a later SF that runs out of time loses nothing)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                json.dump(row, fh, indent=1)


if __name__ == "__main__":
    main()
