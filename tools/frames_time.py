"""Time the receive of self-describing frames (stream.receive_frames_device) beside the
fixed-length receive it stands next to (stream.receive_device, told the length), stage by stage,
and the frame gather kernel beside the torch operations it replaces.  A one-off measurement for
DESIGN.md, not part of bench.py.  Needs a HIP GPU.

Shapes: those of tools/find_time.py (SF7, hop = step // 4, noise of sigma 0.1 over everything) -
  stream    one row of 2^24 samples
  rows      32 channel rows of 2^19 samples
- filled back to back with self-describing frames of one length: 1 payload byte at rate 4/8 with
the CRC, which is 16 data symbols, find_time.py's frame.  The same stream serves both receivers.
Per shape, in milliseconds per call:
  receive_device        stream.receive_device with frame_symbols = 16 (the baseline)
  receive_frames        stream.receive_frames_device with max_symbols = 16, default capacities
  and the second one's stages, each on the inputs the chain gives it:
  scan, candidates, gather_heads, run_heads, decode_header, select, gather_frames, run_frames,
  decode_frame
  gather_kernel         stream.gather_frames_device on the selected frames (gather_frames above)
  gather_torch          what it replaces: stream._gather at the clamped starts, then a
                        torch.where mask of the samples beyond each frame's length
Each figure is the median (with the range) over ``--repeats`` device-event windows of
back-to-back calls on one stream after warm-up, the candidates alternating in the same process
so a drift of the machine shows in all of them.  What the two receivers return is compared
before anything is timed.

Every shape runs in a child process of its own under its own time limit; after a child that
fails or runs out of time nothing more is started.

usage: python tools/frames_time.py [--repeats 5] [--limit 240] [--out file.json]
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
# name: (rows, samples per row, calls per window)
SHAPES = {"stream": (1, 1 << 24, 3), "rows": (32, 1 << 19, 3)}


def measure(name, repeats):
    import torch

    import lora_phy_amd as amd
    from lora_phy_amd import codec, stream

    if not torch.cuda.is_available():
        sys.exit("frames_time.py needs a HIP GPU")
    R, L, calls = SHAPES[name]
    step = 1 << SF
    hop = step // 4
    assert codec.frame_symbols(SF, CR, NBYTES) == DATA
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

    # the two receivers agree on this stream before anything is timed
    fixed = stream.receive_device(plan, x, DATA, hop)
    got = stream.receive_frames_device(plan, x, DATA, hop)
    torch.cuda.synchronize()
    planted = (torch.arange(per_row, device="cuda") * frame_len)[None, :].expand(R, per_row)
    found_fixed = int(fixed.found.count.sum())
    found = int(got.found.count.sum())
    valid = got.found.valid
    at_planted = int((got.found.starts[:, :per_row] == planted)[valid[:, :per_row]].sum())
    ok = int(((got.frames.status.view(R, -1) == codec.FRAME_OK) & valid).sum())
    both = valid[:, :per_row] & fixed.found.valid[:, :per_row]
    same_starts = bool(torch.equal(got.found.starts[:, :per_row], fixed.found.starts[:, :per_row]))
    sym_frames = got.result.symbols.to(torch.int32).view(R, -1, DATA)[:, :per_row]
    sym_fixed = fixed.result.symbols.to(torch.int32).view(R, -1, DATA)[:, :per_row]
    same_symbols = bool(torch.equal(sym_frames[both], sym_fixed[both]))
    cands = int(got.candidates.sum())

    # the chain's stages on the inputs the chain gives them
    met = plan.scan(x, hop)
    ccount, cstarts = stream.find_candidates_device(met, hop, SF, 1, row_len=L)
    C = cstarts.shape[1]
    flat = x.reshape(-1)
    row0 = (torch.arange(R, device="cuda") * L)[:, None]
    hat = torch.where(cstarts >= 0, cstarts + row0, cstarts).reshape(-1)
    hlen = torch.full_like(hat, 10 * step)
    heads = stream.gather_frames_device(flat, hat, hlen, 10 * step)
    hres = plan.run(heads)
    hdr = codec.decode_header(hres.symbols, SF)
    status, hsym = hdr.status.view(R, C), hdr.nsym.view(R, C)
    sel, nsym = stream.select_frames_device(cstarts, status, hsym, step, L, DATA)
    fat = torch.where(sel.starts >= 0, sel.starts + row0, sel.starts).reshape(-1)
    flen = (nsym.reshape(-1).to(torch.int64) + 2) * step
    cut = frame_len
    cutf = stream.gather_frames_device(flat, fat, flen, cut)
    fres = plan.run(cutf)
    navail = nsym.reshape(-1)
    max_bytes = codec.frame_capacity(SF, DATA)
    t_idx = torch.arange(cut, device="cuda")[None, :]

    def gather_torch():
        rows = stream._gather(flat, fat.clamp_min(0), cut)
        return torch.where((t_idx < flen[:, None]) & (fat >= 0)[:, None], rows, torch.zeros((), dtype=rows.dtype,
                                                                                          device="cuda"))

    assert torch.equal(gather_torch(), cutf)

    def window(fn, n):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        for _ in range(n):
            fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) / n

    fns = {"receive_device": lambda: stream.receive_device(plan, x, DATA, hop),
           "receive_frames": lambda: stream.receive_frames_device(plan, x, DATA, hop),
           "scan": lambda: plan.scan(x, hop, out=met),
           "candidates": lambda: stream.find_candidates_device(met, hop, SF, 1, row_len=L),
           "gather_heads": lambda: stream.gather_frames_device(flat, hat, hlen, 10 * step, out=heads),
           "run_heads": lambda: plan.run(heads),
           "decode_header": lambda: codec.decode_header(hres.symbols, SF, out=hdr),
           "select": lambda: stream.select_frames_device(cstarts, status, hsym, step, L, DATA),
           "gather_frames": lambda: stream.gather_frames_device(flat, fat, flen, cut, out=cutf),
           "run_frames": lambda: plan.run(cutf),
           "decode_frame": lambda: codec.decode_frame(fres.symbols, SF, navail, max_bytes),
           "gather_kernel": lambda: stream.gather_frames_device(flat, fat, flen, cut, out=cutf),
           "gather_torch": gather_torch}
    for fn in fns.values():
        window(fn, 1)
    t = {key: [] for key in fns}
    for _ in range(repeats):
        for key, fn in fns.items():
            t[key].append(window(fn, calls))
    row = {"shape": name, "sf": SF, "rows": R, "samples_per_row": L, "hop": hop, "data_symbols": DATA,
           "payload_bytes": NBYTES, "rdd": CR, "sigma": SIGMA, "planted": R * per_row, "found_fixed": found_fixed,
           "found_frames": found, "found_at_planted_starts": at_planted, "status_ok": ok,
           "same_starts_as_fixed": same_starts, "same_symbols_as_fixed": same_symbols, "candidates": cands,
           "candidate_slots": R * C, "frame_slots": int(sel.starts.numel()), "calls_per_window": calls,
           "device": torch.cuda.get_device_name(0)}
    for key, v in t.items():
        row[key + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    row["receive_frames_over_receive_device"] = row["receive_frames_ms"]["median"] / row["receive_device_ms"]["median"]
    row["gather_kernel_over_gather_torch"] = row["gather_kernel_ms"]["median"] / row["gather_torch_ms"]["median"]
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
