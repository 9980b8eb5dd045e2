"""Time the frame finder on the device (lora_find_frames_batch) beside the host finder it
stands next to, and the stream receive with and without the host in it.  A one-off measurement
for DESIGN.md, not part of bench.py.  Needs a HIP GPU.

Shapes (SF7, hop = step // 4, frames of 16 data symbols planted back to back, noise of sigma
0.1 over everything; the planted count is recorded):
  stream    one row of 2^24 samples (tools/scan_time.py's stream)
  rows      32 channel rows of 2^19 samples
Per shape, in milliseconds per call:
  scan             plan.scan into pre-allocated outputs
  find_host        the host finder on the scan's outputs: stream._candidates, the copy of every
                   window's packed start to the host, stream._greedy per row - the body of
                   find_frames / receive_wideband
  find_device      stream.find_frames_device into pre-allocated outputs: one kernel
  receive_host     stream.receive for the stream; for the rows, receive_wideband's body behind
                   its channelizer (scan, the host finder, one gather, one plan.run)
  receive_device   stream.receive_device with the default capacity (every slot demodulated)
  receive_device_cap  the same with capacity = the planted count per row + 8
Each figure is the median (with the range) over ``--repeats`` device-event windows of
back-to-back calls on one stream after warm-up, the paths alternating in the same process so a
drift of the machine shows in all of them.  The host paths synchronise inside, so for them the
wall clock around a ``synchronize`` is reported as well (``*_wall_ms``).  The device and host
results are compared before anything is timed.

Every shape runs in a child process of its own under its own time limit; after a child that
fails or runs out of time nothing more is started.

usage: python tools/find_time.py [--repeats 5] [--limit 240] [--out file.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lora-sdr-lightweight-standalone-library-_amd"))

SF, DATA, SIGMA = 7, 16, 0.1
# name: (rows, samples per row, calls per window)
SHAPES = {"stream": (1, 1 << 24, 3), "rows": (32, 1 << 19, 3)}


def measure(name, repeats):
    import numpy as np
    import torch

    import lora_phy_amd as amd
    from lora_phy_amd import stream

    if not torch.cuda.is_available():
        sys.exit("find_time.py needs a HIP GPU")
    R, L, calls = SHAPES[name]
    step = 1 << SF
    hop = step // 4
    frame_len = (DATA + 2) * step
    per_row = L // frame_len
    g = torch.Generator(device="cpu").manual_seed(SF)
    syms = torch.randint(0, 1 << SF, (R * per_row, DATA), generator=g, dtype=torch.int32)
    frames = amd.modulate(syms.cuda(), SF, 1, 125000, 1.0, 0x12).reshape(R, per_row * frame_len)
    x = torch.zeros((R, L), dtype=torch.complex64, device="cuda")
    x[:, :per_row * frame_len] = frames
    x += SIGMA * torch.randn(x.shape, dtype=torch.complex64, device="cuda")
    del frames
    plan = amd.DemodPlan(SF, dechirp=True)
    N, step, k, sw0, sw1, _ = stream._geometry(hop, SF, 1, DATA, 0x12, 125000)
    met = plan.scan(x, hop)
    W = met.power.shape[1]
    cap_small = per_row + 8
    out = stream.FoundFrames(count=torch.empty(R, dtype=torch.int32, device="cuda"),
                             starts=torch.empty((R, per_row), dtype=torch.int64, device="cuda"),
                             end=torch.empty(R, dtype=torch.int64, device="cuda"))

    def host_find():
        packed = stream._candidates(met.power, met.power_avg, met.index, hop, N, 1, k, sw0, sw1, 0.0)
        packed = packed.cpu().numpy()
        return [stream._greedy(packed[r], hop, step, frame_len, 0, L) for r in range(R)]

    def host_receive():
        if R == 1:
            return stream.receive(plan, x[0], DATA, hop)
        plan.scan(x, hop, out=met)
        found = host_find()
        channel = np.repeat(np.arange(R, dtype=np.int64), [len(s) for s in found])
        at = torch.from_numpy(channel * L + np.concatenate(found)).cuda()
        return at, plan.run(stream._gather(x.reshape(-1), at, frame_len))

    # the two finders agree, and so do the two receives, before anything is timed
    want = host_find()
    got = stream.find_frames_device(met, hop, SF, 1, DATA, row_len=L, out=out)
    torch.cuda.synchronize()
    count = got.count.cpu().numpy()
    assert [int(c) for c in count] == [len(s) for s in want], (count, [len(s) for s in want])
    for r in range(R):
        assert np.array_equal(got.starts[r, :count[r]].cpu().numpy(), want[r]), r
    ref = host_receive()[1]
    dev = stream.receive_device(plan, x, DATA, hop)
    torch.cuda.synchronize()
    assert torch.equal(dev.result.symbols.cpu()[dev.found.valid.reshape(-1).cpu()], ref.symbols.cpu())
    found_frames = int(count.sum())
    right = sum(int(np.isin(np.arange(per_row) * frame_len, s).sum()) for s in want)

    def window(fn, n):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        t0.record()
        for _ in range(n):
            fn()
        t1.record()
        t1.synchronize()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / n, (time.perf_counter() - w0) * 1e3 / n

    fns = {"scan": lambda: plan.scan(x, hop, out=met),
           "find_host": host_find,
           "find_device": lambda: stream.find_frames_device(met, hop, SF, 1, DATA, row_len=L, out=out),
           "receive_host": host_receive,
           "receive_device": lambda: stream.receive_device(plan, x, DATA, hop),
           "receive_device_cap": lambda: stream.receive_device(plan, x, DATA, hop, capacity=cap_small)}
    for fn in fns.values():
        window(fn, 1)
    t = {key: [] for key in fns}
    for _ in range(repeats):
        for key, fn in fns.items():
            t[key].append(window(fn, calls))
    row = {"shape": name, "sf": SF, "rows": R, "samples_per_row": L, "hop": hop, "windows_per_row": W,
           "data_symbols": DATA, "sigma": SIGMA, "planted": R * per_row, "found": found_frames,
           "found_at_planted_starts": right, "calls_per_window": calls, "capacity_default": per_row,
           "capacity_small": cap_small, "device": torch.cuda.get_device_name(0)}
    for key, v in t.items():
        ev = [a for a, _ in v]
        row[key + "_ms"] = {"median": statistics.median(ev), "min": min(ev), "max": max(ev)}
        if key.endswith("_host"):
            wall = [b for _, b in v]
            row[key + "_wall_ms"] = {"median": statistics.median(wall), "min": min(wall), "max": max(wall)}
    row["find_device_over_find_host"] = row["find_device_ms"]["median"] / row["find_host_ms"]["median"]
    row["receive_device_over_receive_host"] = row["receive_device_ms"]["median"] / row["receive_host_ms"]["median"]
    row["receive_device_cap_over_receive_host"] = (row["receive_device_cap_ms"]["median"] /
                                                   row["receive_host_ms"]["median"])
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds each shape's process may take")
    ap.add_argument("--shape", choices=sorted(SHAPES), help="(internal) measure this shape in this process")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.shape:
        return measure(args.shape, args.repeats)
    rows = []
    for name in SHAPES:
        try:
            got = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", name, "--repeats",
                                  str(args.repeats)], capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            sys.exit(f"{name}: no result within {args.limit} s; nothing more is started")
        if got.returncode != 0:
            sys.stderr.write(got.stderr[-4000:])
            sys.exit(f"{name}: exit status {got.returncode}; nothing more is started")
        rows.append(json.loads(got.stdout.strip().splitlines()[-1]))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump({"windows": args.repeats, "shapes": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
