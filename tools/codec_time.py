"""Time the device payload decode (lora_phy_amd.codec.decode) at the project's batch shapes
and the host path (codes.decode_with_crc) over the same symbols.  A one-off measurement for
DESIGN.md, not part of bench.py.  Needs a HIP GPU.

For each shape (frames x symbols per frame) it reports, in microseconds per call:
  * eager   - HIP events around `calls` back-to-back codec.decode calls with the outputs
              pre-allocated, after warm-up (what a Python caller pays per call: the kernel
              or the host's enqueue rate, whichever is slower; the host's own time per call
              to enqueue is reported beside it);
  * graph   - the same calls captured into one HIP graph and replayed (the device side alone:
              kernel plus dispatch, no Python between the launches);
  each as the median and the range over `--repeats` timed windows; and
  * host    - codes.decode_with_crc frame by frame over a 4,096-frame subset, scaled to the
              batch (the host CRC is a Python loop: the full batch would take minutes).

usage: python tools/codec_time.py [--calls 1000] [--repeats 5] [--out file.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lora-sdr-lightweight-standalone-library-_amd"))

SHAPES = ((15625, 64), (1000000, 16))
HOST_SUBSET = 4096
# ms per step of the demodulator on the same batches (profiles/r06/bench_default.json:
# ms_per_step, and extra.channels.ms_per_step)
DEMOD_STEP_MS = {(15625, 64): 0.1877803000388667, (1000000, 16): 3.891995360609144}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch

    from lora_phy_amd import codec, codes

    if not torch.cuda.is_available():
        sys.exit("codec_time.py needs a HIP GPU")
    rows = []
    for F, S in SHAPES:
        gen = torch.Generator("cuda").manual_seed(F + S)
        pay = torch.randint(0, 256, (F, S // 2 - 2), dtype=torch.uint8, device="cuda", generator=gen)
        sym = codec.encode(pay, append_crc=True)
        out = codec.decode(sym)
        torch.cuda.synchronize()
        assert bool(out.crc_ok.all()) and bool((out.payload[:, :S // 2 - 2] == pay).all())

        enqueue = []  # host microseconds per call each window's loop took to enqueue its work

        def window(fn, n):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            h = time.perf_counter()
            fn()
            enqueue.append((time.perf_counter() - h) * 1e6 / n)
            t1.record()
            t1.synchronize()
            return t0.elapsed_time(t1) * 1e3 / n

        def eager():
            for _ in range(args.calls):
                codec.decode(sym, out=out)

        per_graph = 100
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            codec.decode(sym, out=out)
        torch.cuda.current_stream().wait_stream(side)
        with torch.cuda.graph(g):
            for _ in range(per_graph):
                codec.decode(sym, out=out)
        nrep = max(1, args.calls // per_graph)

        def replay():
            for _ in range(nrep):
                g.replay()

        eager()
        replay()
        torch.cuda.synchronize()
        # the two alternate, so a drift of the machine shows in both
        te, tg = [], []
        for _ in range(args.repeats):
            te.append(window(eager, args.calls))
            tg.append(window(replay, nrep * per_graph))

        h_sym = sym[:HOST_SUBSET].cpu().numpy()
        t = time.perf_counter()
        ok = [codes.decode_with_crc(h_sym[f])[1] for f in range(len(h_sym))]
        host_s = (time.perf_counter() - t) * F / len(h_sym)
        assert all(ok)

        step_us = DEMOD_STEP_MS[(F, S)] * 1e3
        row = {"frames": F, "symbols_per_frame": S, "calls_per_window": args.calls,
               "eager_us": {"median": statistics.median(te), "min": min(te), "max": max(te)},
               "graph_us": {"median": statistics.median(tg), "min": min(tg), "max": max(tg)},
               "eager_host_enqueue_us": statistics.median(enqueue[0::2]),
               "demod_step_us": step_us,
               "eager_over_demod_step": statistics.median(te) / step_us,
               "graph_over_demod_step": statistics.median(tg) / step_us,
               "host_decode_with_crc_s": host_s,
               "host_note": f"timed on {len(h_sym)} frames, scaled to {F}"}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "shapes": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
