"""Measure what stream.receive_preamble_frames_device returns from noisy streams of preambled
self-describing frames that went through stream.propagate first (awgn.sweep_receive_preamble with
``propagate=``): the first figures of the preamble chain under fractional timing, a sample-clock
offset, a two-path channel and a carrier drift.  SF 7, 9 and 12, tools/preamble_prob.py's frame
counts, payloads, seeds and SNR points, and the thresholds that tool chose per SF (read from
profiles/stream/preamble_prob.json).  A one-off measurement for DESIGN.md, not a gate and not part
of bench.py: no figure here is a threshold, nobody has measured any of them before.  Needs a HIP GPU.

The channels:
  none          no propagate call: must equal preamble_prob.json's ``preamble`` sweep at offset 0,
                figure for figure (``reproduces_preamble_prob``), which shows the hook changes nothing
  identity      propagate with a delay of 0: a copy, scored by the channel's rule (one chip)
  delay_0.25, delay_0.5
                one path, a quarter and half a sample late; at osr 1 and at osr 2
  sfo_20, sfo_40
                the sample clock off by 20 and 40 ppm
  two_paths     a second path 1.5 samples late at -6 dB with a quarter-turn phase
  drift_100     the carrier drifting by 100 Hz/s at fs = 125 kHz * osr
A planted frame counts as found when a returned start lies within one chip of ``planted + delay +
sfo * planted`` (``sweep_receive_preamble``); ``returned_ok`` asks for the exact payload too.

usage: python tools/propagate_prob.py [--frames 600] [--out file.json]
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
        "p_ok", "false_frames_per_million_windows", "cfo_right")
BASELINE = os.path.join(ROOT, "profiles", "stream", "preamble_prob.json")


def channels(osr):
    from lora_phy_amd import stream

    fs = 125e3 * osr
    both = {"identity": dict(delay=0.0), "delay_0.25": dict(delay=0.25), "delay_0.5": dict(delay=0.5)}
    if osr != 1:
        return dict(none=None, **both)
    return dict(none=None, **both, sfo_20=dict(sfo_ppm=20.0), sfo_40=dict(sfo_ppm=40.0),
                two_paths=dict(delay=[0.0, 1.5], gain=[1.0, 0.5j]),
                drift_100=dict(drift=stream.drift_word(100.0, fs)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--sf", type=int, nargs="*", default=list(SFS))
    ap.add_argument("--osr", type=int, nargs="*", default=[1, 2])
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch

    from lora_phy_amd import awgn

    if not torch.cuda.is_available():
        sys.exit("propagate_prob.py needs a HIP GPU")
    with open(BASELINE) as fh:
        base = json.load(fh)
    chosen = {c["sf"]: c["chosen_thresh_db"] for c in base["threshold_choice"]}
    row = {"device": torch.cuda.get_device_name(0), "hop": "step / 4", "max_bytes": MAX_BYTES, "rdd": CR,
           "frames_per_point": args.frames, "snr_db": SNRS, "preamble": 8, "preamble_acc": 6,
           "thresh_db": {str(sf): chosen[sf] for sf in args.sf}, "sweeps": []}
    for sf in args.sf:
        for osr in args.osr:
            for name, ch in channels(osr).items():
                t0 = time.time()
                recs = awgn.sweep_receive_preamble(sf, SNRS, frames=args.frames, max_bytes=MAX_BYTES, cr=CR, osr=osr,
                                                   thresh_up_db=chosen[sf], thresh_dn_db=chosen[sf], seed=2026 + sf,
                                                   propagate=ch)
                sweep = {"sf": sf, "osr": osr, "channel": name, "propagate": recs[0].get("propagate"),
                         "planted": recs[0]["planted"], "windows": recs[0]["windows"],
                         **{k: [r[k] for r in recs] for k in KEYS}, "seconds": time.time() - t0}
                if name == "none" and osr == 1 and args.frames == base["frames_per_point"]:
                    ref = [s for s in base["sweeps"] if s["sf"] == sf and s["chain"] == "preamble"
                           and s["cfo_bins"] == 0.0]
                    sweep["reproduces_preamble_prob"] = bool(ref) and all(sweep[k] == ref[0][k] for k in KEYS)
                row["sweeps"].append(sweep)
                print(json.dumps(sweep), flush=True)
            if args.out:  # (kept after every shape: a later one that runs out of time loses nothing)
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as fh:
                    json.dump(row, fh, indent=1)


if __name__ == "__main__":
    main()
