"""Time stream.receive_frames_device with soft=True beside soft=False, and the stages that differ,
on tools/frames_time.py's two shapes (SF7, hop = step // 4, noise of sigma 0.1, rows filled back
to back with self-describing frames of 16 data symbols).  A one-off measurement for DESIGN.md, not
part of bench.py.  Needs a HIP GPU.

Per shape, in milliseconds per call:
  receive_hard / receive_soft      the whole chain, soft=False / soft=True (max_flips 5)
  run_heads, soft_bits_heads       plan.run and plan.soft_bits(reduced=(2, 8)) on the candidates' heads
  decode_header, decode_header_soft
  run_frames, soft_bits_frames     the same two on the selected slots
  decode_frame, decode_frame_soft
Each figure is the median (with the range) over ``--repeats`` device-event windows of back-to-back
calls after warm-up, the candidates alternating in one process so a drift of the machine shows in
all of them.  What the two chains return is compared before anything is timed.

Every shape runs in a child process of its own under its own time limit; after a child that
fails or runs out of time nothing more is started.

usage: python tools/frames_soft_time.py [--repeats 5] [--limit 240] [--out file.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lora-sdr-lightweight-standalone-library-_amd"))

SF, DATA, SIGMA, NBYTES, CR = 7, 16, 0.1, 1, 4
SHAPES = {"stream": (1, 1 << 24, 3), "rows": (32, 1 << 19, 3)}


def measure(name, repeats):
    import torch

    import lora_phy_amd as amd
    from lora_phy_amd import codec, stream

    if not torch.cuda.is_available():
        sys.exit("frames_soft_time.py needs a HIP GPU")
    R, L, calls = SHAPES[name]
    step = 1 << SF
    hop = step // 4
    frame_len = (DATA + 2) * step
    per_row = L // frame_len
    g = torch.Generator(device="cpu").manual_seed(SF)
    pay = torch.randint(0, 256, (R * per_row, NBYTES), generator=g, dtype=torch.uint8).cuda()
    syms, _ = codec.encode_frame(pay, None, SF, CR)
    frames = amd.modulate(syms, SF, 1, 125000, 1.0, 0x12).reshape(R, per_row * frame_len)
    x = torch.zeros((R, L), dtype=torch.complex64, device="cuda")
    x[:, :per_row * frame_len] = frames
    x += SIGMA * torch.randn(x.shape, dtype=torch.complex64, device="cuda")
    del frames
    plan = amd.DemodPlan(SF, dechirp=True)

    hard = stream.receive_frames_device(plan, x, DATA, hop)
    soft = stream.receive_frames_device(plan, x, DATA, hop, soft=True)
    torch.cuda.synchronize()
    same = {"starts": bool(torch.equal(hard.found.starts, soft.found.starts)),
            "payload_of_valid": bool(torch.equal(hard.frames.payload[hard.found.valid.reshape(-1)],
                                                 soft.frames.payload[soft.found.valid.reshape(-1)]))}
    ok_hard = int(((hard.frames.status.view(R, -1) == codec.FRAME_OK) & hard.found.valid).sum())
    ok_soft = int(((soft.frames.status.view(R, -1) == codec.FRAME_OK) & soft.found.valid).sum())

    # the stages on the inputs the hard chain gives them
    met = plan.scan(x, hop)
    ccount, cstarts = stream.find_candidates_device(met, hop, SF, 1, row_len=L)
    C = cstarts.shape[1]
    flat = x.reshape(-1)
    row0 = (torch.arange(R, device="cuda") * L)[:, None]
    hat = torch.where(cstarts >= 0, cstarts + row0, cstarts).reshape(-1)
    heads = stream.gather_frames_device(flat, hat, torch.full_like(hat, 10 * step), 10 * step)
    hres = plan.run(heads)
    hllr = plan.soft_bits(heads, hres, reduced=(2, 8))
    hdr = codec.decode_header(hres.symbols, SF)
    sel, nsym = stream.select_frames_device(cstarts, hdr.status.view(R, C), hdr.nsym.view(R, C), step, L, DATA)
    fat = torch.where(sel.starts >= 0, sel.starts + row0, sel.starts).reshape(-1)
    flen = (nsym.reshape(-1).to(torch.int64) + 2) * step
    cutf = stream.gather_frames_device(flat, fat, flen, frame_len)
    fres = plan.run(cutf)
    fllr = plan.soft_bits(cutf, fres, reduced=(2, 8))
    navail = nsym.reshape(-1)
    max_bytes = codec.frame_capacity(SF, DATA)

    def window(fn, n):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        for _ in range(n):
            fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) / n

    fns = {"receive_hard": lambda: stream.receive_frames_device(plan, x, DATA, hop),
           "receive_soft": lambda: stream.receive_frames_device(plan, x, DATA, hop, soft=True),
           "run_heads": lambda: plan.run(heads),
           "soft_bits_heads": lambda: plan.soft_bits(heads, hres, out=hllr, reduced=(2, 8)),
           "decode_header": lambda: codec.decode_header(hres.symbols, SF),
           "decode_header_soft": lambda: codec.decode_header_soft(hllr[:, 2:], SF),
           "run_frames": lambda: plan.run(cutf),
           "soft_bits_frames": lambda: plan.soft_bits(cutf, fres, out=fllr, reduced=(2, 8)),
           "decode_frame": lambda: codec.decode_frame(fres.symbols, SF, navail, max_bytes),
           "decode_frame_soft": lambda: codec.decode_frame_soft(fllr[:, 2:], SF, navail, max_bytes)}
    for fn in fns.values():
        window(fn, 1)
    t = {key: [] for key in fns}
    for _ in range(repeats):
        for key, fn in fns.items():
            t[key].append(window(fn, calls))
    row = {"shape": name, "sf": SF, "rows": R, "samples_per_row": L, "hop": hop, "data_symbols": DATA,
           "payload_bytes": NBYTES, "rdd": CR, "sigma": SIGMA, "planted": R * per_row,
           "found_hard": int(hard.found.count.sum()), "found_soft": int(soft.found.count.sum()),
           "status_ok_hard": ok_hard, "status_ok_soft": ok_soft, "same": same, "candidate_slots": R * C,
           "frame_slots": int(sel.starts.numel()), "calls_per_window": calls, "device": torch.cuda.get_device_name(0)}
    for key, v in t.items():
        row[key + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    med = {k: row[k + "_ms"]["median"] for k in fns}
    row["receive_soft_over_receive_hard"] = med["receive_soft"] / med["receive_hard"]
    row["soft_bits_over_run_heads"] = med["soft_bits_heads"] / med["run_heads"]
    row["soft_bits_over_run_frames"] = med["soft_bits_frames"] / med["run_frames"]
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
