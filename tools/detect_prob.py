"""Measure the stream receiver's detection probability (awgn.sweep_receive): frames planted at
known starts, impaired on the device by stream.impair (counter-based AWGN, reproducible on the
CPU) and received by stream.receive_device with hop = step / 4 and the default thresh_db.  SF 7, 9
and 12 at osr 1, SNR -20 .. +5 dB in 1 dB steps, ``--frames`` planted frames of 16 symbols per
point, at a carrier offset of 0 and of 0.25 bin, and at least ``--noise-windows`` windows of noise
alone per SF for the false starts.  A one-off measurement for DESIGN.md, not a gate and not part of
bench.py.  Needs a HIP GPU.

Recorded per point: detection probability (planted starts returned exactly), false starts per
10^6 windows, and the all-symbols-correct rate among detected frames.

usage: python tools/detect_prob.py [--frames 2000] [--noise-windows 10000000] [--out file.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lora-sdr-lightweight-standalone-library-_amd"))

SFS = (7, 9, 12)
SNRS = list(range(-20, 6))
CFOS = (0.0, 0.25)
SYMBOLS = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--noise-windows", type=int, default=10_000_000)
    ap.add_argument("--sf", type=int, nargs="*", default=list(SFS))
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch

    from lora_phy_amd import awgn

    if not torch.cuda.is_available():
        sys.exit("detect_prob.py needs a HIP GPU")
    row = {"device": torch.cuda.get_device_name(0), "osr": 1, "frame_symbols": SYMBOLS, "hop": "step / 4",
           "thresh_db": 0.0, "frames_per_point": args.frames, "snr_db": SNRS, "sweeps": [], "noise_only": []}
    for sf in args.sf:
        for cfo in CFOS:
            t0 = time.time()
            recs = awgn.sweep_receive(sf, SNRS, frames=args.frames, frame_symbols=SYMBOLS, cfo_bins=cfo,
                                      seed=2026 + sf, noise_windows=args.noise_windows if cfo == 0.0 else 0)
            if recs and recs[-1].get("noise_only"):
                row["noise_only"].append(recs.pop())
            row["sweeps"].append({
                "sf": sf, "cfo_bins": cfo, "planted": recs[0]["planted"], "windows": recs[0]["windows"],
                "p_detect": [r["p_detect"] for r in recs],
                "false_starts_per_million_windows": [r["false_starts"] * 1e6 / r["windows"] for r in recs],
                "p_all_correct_given_detected": [r["p_all_correct_given_detected"] for r in recs],
                "detected": [r["detected"] for r in recs], "false_starts": [r["false_starts"] for r in recs],
                "all_symbols_correct": [r["all_symbols_correct"] for r in recs], "seconds": time.time() - t0})
            print(json.dumps(row["sweeps"][-1]), flush=True)
    print(json.dumps(row["noise_only"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(row, fh, indent=1)


if __name__ == "__main__":
    main()
