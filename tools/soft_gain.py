"""Frame-error rates of the hard and the soft receive chain on the GPU path, side by side:
LoRaMod.work_payload(chain="lora") -> white noise -> LoRaDemod.work_payload(chain="lora")
against LoRaDemod.work_payload_soft on the same IQ.  SF 7 / 9 / 12, CR 4/5 and 4/8, 1 dB steps
around each waterfall, `--frames` seeded frames of 16 payload bytes per point.  A one-off
measurement for DESIGN.md, not part of bench.py.  Needs a HIP GPU.

Noise: a unit-amplitude signal plus sigma = 10^(-snr_db/20) on I and on Q each (seeded, drawn
on the device), the convention of the model that motivated the soft path and of
tests/soft_checker.noise_sigma.  awgn.sweep_chain divides that sigma by sqrt(2): a point here
carries the noise of sweep_chain's point 3.01 dB lower, recorded as `snr_db_sweep_chain`.

usage: python tools/soft_gain.py [--frames 1000] [--seed 2026] [--out profiles/soft/soft_gain.json]
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lora-sdr-lightweight-standalone-library-_amd"))

# sf -> the middle of the sweep, dB (three 1 dB steps to either side)
CENTRE = {7: -7, 9: -13, 12: -21}
RATES = (1, 4)  # RDD: coding rates 4/5 and 4/8
NBYTES = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "soft", "soft_gain.json"))
    args = ap.parse_args()

    import torch

    import lora_phy_amd as amd

    if not torch.cuda.is_available():
        sys.exit("soft_gain.py needs a HIP GPU")
    dev = torch.device("cuda", 0)
    points = []
    for sf, centre in CENTRE.items():
        for rdd in RATES:
            cr = f"4/{4 + rdd}"
            g = torch.Generator(device="cpu").manual_seed(args.seed + 16 * sf + rdd)
            pay = torch.randint(0, 256, (args.frames, NBYTES), generator=g, dtype=torch.uint8).to(dev)
            clean = amd.LoRaMod(sf, cr=rdd).work_payload(pay, chain="lora")
            demod = amd.LoRaDemod(sf, cr=rdd)
            quiet = demod.work_payload_soft(clean, NBYTES)
            assert torch.equal(quiet.payload, pay) and int(quiet.errors.abs().sum()) == 0
            gen = torch.Generator(device=dev).manual_seed(args.seed + 1000 * sf + rdd)
            for snr in range(centre - 3, centre + 4):
                sigma = 10.0 ** (-snr / 20.0)
                noise = torch.randn(clean.shape + (2,), generator=gen, device=dev) * sigma
                iq = clean + torch.view_as_complex(noise)
                hard = demod.work_payload(iq, NBYTES, chain="lora")
                soft = demod.work_payload_soft(iq, NBYTES)
                hard_bad = int((hard.payload != pay).any(dim=1).sum())
                soft_bad = int((soft.payload != pay).any(dim=1).sum())
                row = {"sf": sf, "cr": cr, "snr_db": snr, "snr_db_sweep_chain": snr - 20 * math.log10(math.sqrt(2.0)),
                       "sigma_per_component": sigma, "frames": args.frames, "payload_bytes": NBYTES,
                       "symbols_per_frame": int(demod.last.symbols.shape[1]) + 2,
                       "hard_bad": hard_bad, "soft_bad": soft_bad,
                       "hard_fer": hard_bad / args.frames, "soft_fer": soft_bad / args.frames,
                       "sync_ok": float(demod.sync_ok().float().mean())}
                points.append(row)
                print(json.dumps(row), flush=True)
            del clean, demod
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "seed": args.seed, "points": points}, fh, indent=1)


if __name__ == "__main__":
    main()
