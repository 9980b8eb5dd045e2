"""Time the soft bits (DemodPlan.soft_bits) beside the detector metrics (DemodPlan.detect_metrics)
and the demodulator's own step (DemodPlan.run) at the project's batch shapes: BASELINE.json
configs[1] (SF7) and configs[2] (SF12), 15,625 frames of 2 + 64 symbols each, generated on the
device as bench.py generates them - the shapes of tools/metrics_time.py.  Also the soft chain
decoder (codec.decode_chain_soft) beside the hard one (codec.decode_chain) on the same frames'
data columns at CR 4/8.  A one-off measurement for DESIGN.md, not part of bench.py.  Needs a
HIP GPU.

Per shape, in milliseconds per call, every output pre-allocated: the median (with the range)
over `--repeats` device-event windows of back-to-back calls on one stream after warm-up, the
calls alternating in the same process so a drift of the machine shows in all of them; and the
ratios soft_bits / detect_metrics and soft_bits / run.

usage: python tools/soft_time.py [--repeats 5] [--frames 15625] [--out profiles/soft/soft_time.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lora-sdr-lightweight-standalone-library-_amd"))

# (sf, data symbols per frame, calls per window of soft_bits / detect_metrics, of plan.run, of the decoders)
SHAPES = ((7, 64, 20, 100, 100), (12, 64, 3, 10, 100))
RDD = 4


def stats(ts, calls):
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts), "calls_per_window": calls}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=15625)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "soft", "soft_time.json"))
    args = ap.parse_args()

    import torch

    import lora_phy_amd as amd
    from lora_phy_amd import codec

    if not torch.cuda.is_available():
        sys.exit("soft_time.py needs a HIP GPU")
    rows = []
    for sf, data_syms, n_met, n_run, n_dec in SHAPES:
        g = torch.Generator(device="cpu").manual_seed(sf)
        syms = torch.randint(0, 1 << sf, (args.frames, data_syms), generator=g, dtype=torch.int32)
        iq = amd.modulate(syms.cuda(), sf, 1, 125000, 1.0, 0x12)
        plan = amd.DemodPlan(sf, dechirp=True)
        res = plan.run(iq)
        met = plan.detect_metrics(iq, res)
        llr = plan.soft_bits(iq, res)
        nbytes = codec.chain_capacity(sf, RDD, data_syms)
        hard = codec.decode_chain(res.symbols, sf, RDD, nbytes)
        soft = codec.decode_chain_soft(llr[:, 2:], sf, RDD, nbytes)
        torch.cuda.synchronize()
        got = res.symbols.cpu().numpy()
        assert (got == syms.numpy()).all() and (met.index.cpu().numpy()[:, 2:] == got).all()
        # noiseless frames: the signs are the symbols' bits, so without a code both decoders agree
        # (the random symbols are no codewords, so at RDD 4 the two need not)
        n0 = codec.chain_capacity(sf, 0, data_syms)
        assert torch.equal(codec.decode_chain(res.symbols, sf, 0, n0).payload,
                           codec.decode_chain_soft(llr[:, 2:], sf, 0, n0).payload)

        def window(fn, n):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(n):
                fn()
            t1.record()
            t1.synchronize()
            return t0.elapsed_time(t1) / n

        fns = {
            "soft_bits_ms": (lambda: plan.soft_bits(iq, res, out=llr), n_met),
            "detect_metrics_ms": (lambda: plan.detect_metrics(iq, res, out=met), n_met),
            "plan_run_ms": (lambda: plan.run(iq, out=res), n_run),
            "decode_chain_soft_ms": (lambda: codec.decode_chain_soft(llr[:, 2:], sf, RDD, nbytes, out=soft), n_dec),
            "decode_chain_ms": (lambda: codec.decode_chain(res.symbols, sf, RDD, nbytes, out=hard), n_dec),
        }
        for fn, n in fns.values():
            window(fn, 2)
        ts = {k: [] for k in fns}
        for _ in range(args.repeats):
            for k, (fn, n) in fns.items():
                ts[k].append(window(fn, n))
        row = {"sf": sf, "frames": args.frames, "symbols_per_frame": data_syms + 2, "rdd": RDD,
               "payload_bytes": nbytes}
        for k, (fn, n) in fns.items():
            row[k] = stats(ts[k], n)
        med = {k: row[k]["median"] for k in fns}
        row["soft_bits_over_detect_metrics"] = med["soft_bits_ms"] / med["detect_metrics_ms"]
        row["soft_bits_over_run"] = med["soft_bits_ms"] / med["plan_run_ms"]
        row["decode_soft_over_hard"] = med["decode_chain_soft_ms"] / med["decode_chain_ms"]
        row["soft_bits_Msymbols_per_s"] = args.frames * (data_syms + 2) / med["soft_bits_ms"] / 1e3
        rows.append(row)
        print(json.dumps(row), flush=True)
        del iq, res, met, llr, plan, hard, soft
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "windows": args.repeats, "shapes": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
