"""Time the accumulating scan (DemodPlan.scan_acc) beside the unchanged plain scan, and the
preambled receive chain (stream.receive_preamble_frames_device) beside the receive of
self-describing frames without a preamble (stream.receive_frames_device), stage by stage.  A
one-off measurement for DESIGN.md, not part of bench.py.  Needs a HIP GPU.

Scan shapes (tools/scan_time.py's): one stream of 2^24 samples, SF7 hop 32 and SF12 hop 1024, a
dechirping plan.  Per shape, in milliseconds per call: ``scan`` (plan.scan, the yardstick) and
``scan_acc`` at acc 1, 2 and 6.  The accumulating kernel recomputes the acc spectra of every
output window, so acc times the plain scan is what it is expected to cost.

Chain shapes (tools/frames_time.py's): SF7, hop = step // 4, noise of sigma 0.1 over everything,
one row of 2^24 samples and 32 rows of 2^19, filled back to back with frames of 1 payload byte at
rate 4/8 with the CRC (16 data symbols).  ``receive_frames`` sees them without preamble,
``receive_preamble`` with a preamble of 8 and the delimiter (so fewer frames fit), both with
default capacities and thresholds of 0 dB; then the second chain's stages, each on the inputs the
chain gives it.

Each figure is the median (with the range) over ``--repeats`` device-event windows of
back-to-back calls on one stream after warm-up, the candidates alternating in the same process.
Every shape runs in a child process of its own under its own time limit; after a child that fails
or runs out of time nothing more is started.

usage: python tools/preamble_time.py [--repeats 5] [--limit 240] [--out file.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lora-sdr-lightweight-standalone-library-_amd"))

# name: (sf, hop, calls per window)
SCAN_SHAPES = {"scan_sf7": (7, 32, 10), "scan_sf12": (12, 1024, 3)}
SF, DATA, SIGMA, NBYTES, CR, PRE, ACC = 7, 16, 0.1, 1, 4, 8, 6
# name: (rows, samples per row, calls per window)
CHAIN_SHAPES = {"stream": (1, 1 << 24, 3), "rows": (32, 1 << 19, 3)}


def window(torch, fn, n):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(n):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / n


def timed(torch, fns, calls, repeats):
    for fn in fns.values():
        window(torch, fn, 2)
    t = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            t[k].append(window(torch, fn, calls))
    return {k + "_ms": {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in t.items()}


def measure_scan(name, repeats):
    import torch

    import lora_phy_amd as amd

    sf, hop, calls = SCAN_SHAPES[name]
    step, samples = 1 << sf, 1 << 24
    F = -(-samples // (66 * step))
    g = torch.Generator(device="cpu").manual_seed(sf)
    syms = torch.randint(0, 1 << sf, (F, 64), generator=g, dtype=torch.int32)
    x = amd.modulate(syms.cuda(), sf).reshape(-1)[:samples].clone()
    x += 0.1 * torch.randn(samples, dtype=torch.complex64, device="cuda")
    plan = amd.DemodPlan(sf, dechirp=True, mode="raw")
    met = plan.scan(x, hop)
    one = plan.scan_acc(x, hop, 1)
    torch.cuda.synchronize()
    for k in ("power", "power_avg"):
        assert torch.equal(getattr(met, k).view(torch.int32), getattr(one, k).view(torch.int32)), k
    assert torch.equal(met.index.to(torch.int32), one.index.to(torch.int32))
    fns = {"scan": lambda: plan.scan(x, hop, out=met)}
    for acc in (1, 2, 6):  # (outputs pre-allocated, as the yardstick's)
        kept = plan.scan_acc(x, hop, acc)
        fns["scan_acc%d" % acc] = (lambda a, o: lambda: plan.scan_acc(x, hop, a, out=o))(acc, kept)
    row = {"shape": name, "sf": sf, "samples": samples, "hop": hop, "windows": met.power.shape[1],
           "calls_per_window": calls, "device": torch.cuda.get_device_name(0)}
    row.update(timed(torch, fns, calls, repeats))
    base = row["scan_ms"]["median"]
    for acc in (1, 2, 6):
        r = row["scan_acc%d_ms" % acc]
        row["scan_acc%d_over_scan" % acc] = r["median"] / base
        row["scan_acc%d_max_below_acc_times_scan" % acc] = bool(r["max"] < acc * base) if acc > 1 else None
    row["scan_acc1_within_scan_range"] = bool(row["scan_ms"]["min"] <= row["scan_acc1_ms"]["median"]
                                              <= row["scan_ms"]["max"])
    return row


def measure_chain(name, repeats):
    import torch

    import lora_phy_amd as amd
    from lora_phy_amd import codec, stream

    R, L, calls = CHAIN_SHAPES[name]
    step = 1 << SF
    hop, tail = step // 4, 9 * step // 4
    g = torch.Generator(device="cpu").manual_seed(SF)

    def fill(frame_of, frame_len):
        per_row = L // frame_len
        pay = torch.randint(0, 256, (R * per_row, NBYTES), generator=g, dtype=torch.uint8).cuda()
        syms, _ = codec.encode_frame(pay, None, SF, CR)
        x = torch.zeros((R, L), dtype=torch.complex64, device="cuda")
        x[:, :per_row * frame_len] = frame_of(syms).reshape(R, per_row * frame_len)
        x += SIGMA * torch.randn(x.shape, dtype=torch.complex64, device="cuda")
        return x, per_row

    plain_len = (DATA + 2) * step
    pre_len = (PRE + 2 + DATA) * step + tail
    xa, per_a = fill(lambda s: amd.modulate(s, SF), plain_len)
    xb, per_b = fill(lambda s: amd.modulate_preamble(s, SF, preamble=PRE), pre_len)
    plan = amd.DemodPlan(SF, dechirp=True)
    a = stream.receive_frames_device(plan, xa, DATA, hop)
    b = stream.receive_preamble_frames_device(plan, xb, DATA, ACC, hop, thresh_up_db=0.0, thresh_dn_db=0.0)
    torch.cuda.synchronize()
    planted_b = (torch.arange(per_b, device="cuda") * pre_len + PRE * step)[None, :].expand(R, per_b)
    row = {"shape": name, "sf": SF, "rows": R, "samples_per_row": L, "hop": hop, "sigma": SIGMA,
           "calls_per_window": calls, "device": torch.cuda.get_device_name(0),
           "frames_planted": R * per_a, "frames_found": int(a.found.count.sum()),
           "frames_ok": int(((a.frames.status.view(R, -1) == codec.FRAME_OK) & a.found.valid).sum()),
           "preamble_planted": R * per_b, "preamble_found": int(b.found.count.sum()),
           "preamble_at_planted_starts": int((b.found.starts[:, :per_b] == planted_b)[b.found.valid[:, :per_b]].sum()),
           "preamble_ok": int(((b.frames.status.view(R, -1) == codec.FRAME_OK) & b.found.valid).sum()),
           "preamble_candidates": int(b.candidates.sum()), "frames_candidates": int(a.candidates.sum())}

    up = plan.scan_acc(xb, hop, ACC)
    dn = plan.scan_acc(xb, hop, 2, conj=True)
    ccount, cstarts, ccfo = stream.find_preamble_device(up, dn, hop, SF, 1, ACC, row_len=L)
    C = cstarts.shape[1]
    status = torch.zeros((R, C), dtype=torch.int32, device="cuda")
    hsym = torch.full((R, C), DATA, dtype=torch.int32, device="cuda")
    fns = {"receive_frames": lambda: stream.receive_frames_device(plan, xa, DATA, hop),
           "receive_preamble": lambda: stream.receive_preamble_frames_device(plan, xb, DATA, ACC, hop,
                                                                             thresh_up_db=0.0, thresh_dn_db=0.0),
           "scan_plain": lambda: plan.scan(xb, hop),
           "scan_up": lambda: plan.scan_acc(xb, hop, ACC),
           "scan_dn": lambda: plan.scan_acc(xb, hop, 2, conj=True),
           "find_preamble": lambda: stream.find_preamble_device(up, dn, hop, SF, 1, ACC, row_len=L),
           "select_preamble": lambda: stream.select_preamble_device(cstarts, ccfo, status, hsym, step, L, DATA)}
    row.update(timed(torch, fns, calls, repeats))
    row["receive_preamble_over_receive_frames"] = (row["receive_preamble_ms"]["median"] /
                                                   row["receive_frames_ms"]["median"])
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240)
    ap.add_argument("--out")
    ap.add_argument("--child")
    args = ap.parse_args()
    if args.child:
        fn = measure_scan if args.child in SCAN_SHAPES else measure_chain
        print("RESULT " + json.dumps(fn(args.child, args.repeats)), flush=True)
        return
    rows = []
    for name in list(SCAN_SHAPES) + list(CHAIN_SHAPES):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--repeats",
                                str(args.repeats)], capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            sys.exit(f"{name}: no result within {args.limit} s; nothing more is started")
        got = [ln[7:] for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not got:
            sys.exit(f"{name}: child failed (rc {p.returncode}); nothing more is started\n{p.stderr[-2000:]}")
        rows.append(json.loads(got[0]))
        print(got[0], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump({"windows": args.repeats, "shapes": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
