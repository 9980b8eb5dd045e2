"""How much of the certification's rounding bound the speculative symbol pass uses (DESIGN.md
§3.4): for every loop of the pass (tests/cert_checker.VARIANTS) and the four input batches of
tests/test_gpu_cert.py, the worst |recorded margin - float64 margin| / (n1 (e_spec + E)) - a
margin is the difference of two bins, so the bound allows 2 - and, from the CPU oracle alone,
the worst |X32 - X64| / (E sum|y|) of the reference's transform per SF (the bound allows 1).
Reuses the test's checker; a measurement for DESIGN.md, not part of bench.py.  Needs a HIP GPU.

usage: python tools/cert_slack.py [--out profiles/spec/cert_slack.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "lora-sdr-lightweight-standalone-library-_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spec", "cert_slack.json"))
    args = ap.parse_args()

    import torch

    import lora_phy_amd as amd
    from oracle.pyoracle import Oracle
    from tests import cert_checker as cc

    if not torch.cuda.is_available():
        sys.exit("cert_slack.py needs a HIP GPU")
    O = Oracle()
    variants = []
    for v in cc.VARIANTS:
        mode, sf, osr, window, dechirp = v
        row = {"variant": cc.variant_id(v), "mode": mode, "sf": sf, "osr": osr, "window": window,
               "fused_dechirp": dechirp, "symbols": 0, "listed": 0, "over_bound": 0, "families": {}}
        for family in cc.FAMILIES:
            x, deltas = cc.family_frames(O, v, family)
            plan = amd.DemodPlan(sf, osr, 125000, window, dechirp=dechirp, mode=mode)
            res = plan.run(torch.from_numpy(x).cuda())
            torch.cuda.synchronize()
            rep = cc.evaluate(O, v, x, res.symbols.cpu().numpy(), plan.spec_trace(), deltas)
            row["families"][family] = round(rep["worst"], 5)
            row["symbols"] += x.shape[0] * (x.shape[1] // ((1 << sf) * osr))
            row["listed"] += len(rep["listed"])
            row["over_bound"] += len(rep["over"])
        row["worst_margin_error_over_n1_espec_E"] = max(row["families"].values())
        variants.append(row)
        print(row["variant"], row["worst_margin_error_over_n1_espec_E"], flush=True)
    share = [{"sf": sf, "hann": hann, "worst_bin_error_over_E_sum_y": round(cc.reference_share(O, sf, hann), 5)}
             for sf in range(6, 13) for hann in (False, True)]
    out = {
        "what": "share of the certification bound in use: margin error of k_spec_demod against a float64 "
                "transform of the same window, in units of n1 (e_spec + E) (allowed: 2), and the CPU oracle's "
                "fp32 transform against float64, in units of E sum|y| (allowed: 1)",
        "device": torch.cuda.get_device_name(0),
        "frames_per_batch": {"sf<=9": 5, "sf>=10": 3}, "symbols_per_frame": cc.S_TOTAL,
        "worst_variant": max(v["worst_margin_error_over_n1_espec_E"] for v in variants),
        "worst_reference": max(s["worst_bin_error_over_E_sum_y"] for s in share),
        "variants": variants,
        "reference_share": share,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(f"worst variant {out['worst_variant']}, worst reference {out['worst_reference']} -> {args.out}")


if __name__ == "__main__":
    main()
