"""Host model of the speculative pipeline's certification, float64 numpy.

*** TEST INFRASTRUCTURE ONLY. ***  tests/test_cert_checker.py checks the model against the CPU
oracle, tests/test_gpu_cert.py the kernels against the model, tools/cert_slack.py records how
much of the rounding bound the symbol pass uses.

The pipeline keeps a speculative symbol only if its margin d = |X1| - |X2| exceeds 4 B + 2^-60,
B = n1 (|drate| N + e_ref + e_spec + 2 E), n1 = 2 N max(|I|,|Q|) over the symbol's window.

* ``certified`` restates that test (certify_list / k_est_fast<.., 2> for LEGACY and API,
  k_cert_raw for RAW) with the kernels' double operations in the kernels' order, on the fp32
  values ``DemodPlan.spec_trace()`` returns: its verdict is the kernel's, not an estimate of it.
* ``margin_f64`` is the margin the symbol pass approximates: the window times the exact
  e^{i r' i} (r' the fp32 pre-pass rate as a double), the Hann table if any, a complex128 FFT.
* ``window_max`` / ``slot_max`` are the maxima stage 2 assembles the frame's from.
* ``windows`` cuts a frame into the windows the symbol pass reads; ``sweep_frames`` and
  ``offset_frames`` are the two input families of the GPU test, ``VARIANTS`` its cases.
"""
import numpy as np

U = 1.0 / 16777216.0      # fp32 unit roundoff 2^-24
HW_SINCOS_ERR = 2.0e-7    # lora_demod_fast.hip kHwSinCosErr
SYNC_PAIR = 0xFFFFFFFF    # the reject list's entry for a frame's sync word

# one delta per data symbol of the near-tie sweep: 0 and +-2^-6 .. +-2^-24
DELTAS = [0.0] + [sg * 2.0 ** -k for k in range(6, 25) for sg in (1.0, -1.0)]
S_TOTAL = 39  # symbols per frame: 37 data symbols, a partial last block and certify round
PAD = 3       # samples between the rows: windows start off a 16-byte line

# (mode, sf, osr, window, dechirp): one case per loop of the symbol pass
VARIANTS = (
    [("legacy", sf, 1, w, d) for d in (False, True)
     for sf, w in [(7, "none"), (6, "none"), (8, "none"), (9, "none"), (7, "hann"),
                   (10, "none"), (11, "none"), (12, "none"), (12, "hann")]]
    + [("legacy", sf, osr, "none", d) for d in (False, True) for sf, osr in [(7, 2), (7, 3), (7, 4), (10, 2)]]
    + [("api", 7, 1, "none", True), ("api", 10, 1, "none", True)]
    + [("raw", 6, 1, "none", False), ("raw", 7, 1, "none", True), ("raw", 9, 1, "none", False)])


def variant_id(v):
    mode, sf, osr, window, dechirp = v
    return f"{mode}-sf{sf}-osr{osr}-{window}-{'fused' if dechirp else 'plain'}"


def frames_of(sf):
    """Frames per batch: a stage-2 wave holds several frames plus a ragged one."""
    return 5 if sf <= 9 else 3


# ---- the bound ---------------------------------------------------------------------------

def bound_terms(sf, rate, rate_spec, t_off):
    """(E, e_spec, rmax, drate, tabs) of a frame as certify_list computes them (doubles from the
    fp32 rates and the integer t_off)."""
    N = 1 << sf
    T = N // 16 if N >= 16 else 1
    rate, rate_spec = float(np.float32(rate)), float(np.float32(rate_spec))
    E = (8.0 * sf + 42.0) * U
    drate = abs(rate - rate_spec)
    rmax = max(abs(rate), abs(rate_spec))
    tabs = float(abs(int(t_off)))
    e_spec = 36.0 * U * rmax * T + 16.0 * (1.87e-7 + 1.4143 * HW_SINCOS_ERR) + 2.6e-6 + 9.6e-7
    return E, e_spec, rmax, drate, tabs


def bound(wmax, s, sf, rate, rate_spec, t_off):
    """B of symbol s (its index in the frame) whose window's max(|I|,|Q|) is wmax."""
    N = 1 << sf
    E, e_spec, rmax, drate, tabs = bound_terms(sf, rate, rate_spec, t_off)
    n1 = 2.0 * N * float(wmax)
    L = float(s + 1) * N + tabs
    e_ref = U * rmax * (L + 2.0 * N)
    return n1 * (drate * N + e_ref + e_spec + 2.0 * E)


def certified(d, wmax, s, fp, fp_spec, sf, mode):
    """The kernels' verdict on symbol s of a frame: margin d (fp32), the window's maximum wmax
    (fp32; a LEGACY sync symbol's: the frame's slot), fp / fp_spec the frame's exact and
    speculative offsets (records with rate and t_off).  RAW: no offsets, rate 0 (k_cert_raw);
    LEGACY / API: a frame whose two time offsets differ certifies nothing (same_t)."""
    if mode == "raw":
        return float(d) > 4.0 * bound(wmax, s, sf, 0.0, 0.0, 0) + 2.0 ** -60
    same_t = int(fp["t_off"]) == int(fp_spec["t_off"])
    B = bound(wmax, s, sf, fp["rate"], fp_spec["rate"], fp["t_off"])
    return bool(same_t and float(d) > 4.0 * B + 2.0 ** -60)


# ---- what the symbol pass approximates ---------------------------------------------------

def hann_table(N):
    """0.5 - 0.5 cos(2 pi i / (N - 1)) rounded as the plan's fp32 table is (the cosine correctly
    rounded; the library's cosf may differ from it in a last bit, 2^-24 of a window value)."""
    i = np.arange(N, dtype=np.float32)
    arg = (np.float32(2.0) * np.float32(np.pi) * i / (np.float32(N) - np.float32(1.0))).astype(np.float32)
    c = np.cos(arg.astype(np.float64)).astype(np.float32)
    return (np.float32(0.5) - np.float32(0.5) * c).astype(np.float32)


def spectrum_f64(points, rate=0.0, hann=None):
    z = np.asarray(points).astype(np.complex128)
    if rate != 0.0:
        z = z * np.exp(1j * float(np.float32(rate)) * np.arange(len(z)))
    if hann is not None:
        z = z * np.asarray(hann, np.float64)
    return np.fft.fft(z)


def margin_f64(points, rate=0.0, hann=None):
    """(top |X| - runner-up |X|, argmax) of the window's N points as the symbol pass reads them
    (the oracle's dechirped fp32 samples, every osr-th one), rotated by the exact e^{i rate i}."""
    m = np.abs(spectrum_f64(points, rate, hann))
    k = int(np.argmax(m))
    top = m[k]
    m[k] = -1.0
    return float(top - m.max()), k


def window_max(samples):
    """max(|I|,|Q|) over every sample of a window, as fp32 bits."""
    v = np.ascontiguousarray(np.asarray(samples, np.complex64)).view(np.float32)
    return int(np.abs(v).max().view(np.uint32)) if v.size else 0


def sym_base(s, step, frame_len, t_off):
    """Window start of symbol s under the time-offset rule (LoRaDemod.cpp:142-149)."""
    base = s * step
    if t_off > 0 and base + t_off + step <= frame_len:
        base += t_off
    elif t_off < 0 and -t_off <= base:
        base += t_off
    return base


def windows(O, row, sf, osr, mode, dechirp, t_off):
    """The windows of every symbol of one frame as the symbol pass reads them with the integer
    time offset t_off: a list of complex64 [step] arrays (the N points are ``w[::osr]``).
    legacy / raw: the caller's dechirp (the oracle's fp32 product) when the plan fuses it, else
    the input as it is; api: each window times a fresh down-chirp (phy.cpp:211-225)."""
    N = 1 << sf
    step = N * osr
    L = len(row)
    total = L // step
    if mode == "api":
        return [O.dechirp(row[b:b + step], sf, osr) for b in (sym_base(s, step, L, t_off) for s in range(total))]
    xd = O.dechirp(row, sf, osr) if dechirp else np.asarray(row, np.complex64)
    if mode == "raw":
        t_off = 0
    return [xd[b:b + step] for b in (sym_base(s, step, L, t_off) for s in range(total))]


def slot_max(O, row, sf, osr, dechirp, t_off):
    """The pre-pass's slot, fp32 bits: max(|I|,|Q|) over the samples
    outside the data windows of t_off - [0, 2 step), a positive t_off's [2 step, 2 step +
    t_off), the tail after the last window - of a LEGACY frame."""
    step = (1 << sf) * osr
    L = len(row)
    total = L // step
    xd = O.dechirp(row, sf, osr) if dechirp else np.asarray(row, np.complex64)
    b2 = sym_base(2, step, L, t_off)
    xend = sym_base(total - 1, step, L, t_off) + step
    return window_max(np.concatenate([xd[:max(b2, 2 * step)], xd[xend:]]))


# ---- the input families ------------------------------------------------------------------

def tone(n_samples, k, N, osr, amp=1.0, ph=0.0):
    n = np.arange(n_samples)
    return amp * np.exp(1j * (2 * np.pi * k * n / (N * osr) + ph))


def down_chirp(O, sf, osr):
    """The caller-side dechirp table: 1 x down is exact in the oracle's product."""
    return O.dechirp(np.ones((1 << sf) * osr, np.complex64), sf, osr).astype(np.complex128)


def sweep_frames(O, sf, osr, F, amp=1.0, chirped_sync=True):
    """Family (a), the near-tie sweep, as RAW input (before the caller's dechirp): per frame a
    bin-0 sync pair at 1.7 amp (no rotation, rescaled when amp = 1) and 37 two-tone data symbols
    tone(a, 1.3) + tone(b, 1.3 (1 + delta), phase 0.7), a = (5 + 3 f) mod N, b = (N/2 + 9 + 7 f)
    mod N, one delta of DELTAS per symbol (rotated by 13 per frame, so three frames hold them
    all).  Returns (frames [F, L] complex64, deltas [F, 37]).  chirped_sync=False leaves the
    sync pair un-chirped (LORA_MODE_API estimates on the raw samples, phy.cpp:91-99)."""
    N = 1 << sf
    step = N * osr
    up = np.conj(down_chirp(O, sf, osr))
    out = np.zeros((F, S_TOTAL * step), np.complex64)
    deltas = np.zeros((F, S_TOTAL - 2))
    for f in range(F):
        a, b = (5 + 3 * f) % N, (N // 2 + 9 + 7 * f) % N
        for s in range(S_TOTAL):
            if s < 2:
                y = tone(step, 0, N, osr, 1.7 * amp)
                if not chirped_sync:
                    out[f, s * step:(s + 1) * step] = y.astype(np.complex64)
                    continue
            else:
                dl = DELTAS[(s - 2 + 13 * f) % len(DELTAS)]
                deltas[f, s - 2] = dl
                y = tone(step, a, N, osr, 1.3 * amp) + tone(step, b, N, osr, 1.3 * amp * (1.0 + dl), 0.7)
            out[f, s * step:(s + 1) * step] = (y * up).astype(np.complex64)
    return out, deltas


def t_off_of(toff):
    return int(np.round(np.float32(toff)))


def prepass_t_off(O, row, sf, osr, hann):
    """The integer time offset the pre-pass takes for a LEGACY frame (`row` dechirped), by the
    oracle: the estimate of symbols 0/1 alone - at SF 6-9, osr 1 normalised by those two
    symbols' own maximum (k_est_split's scale guess: the oracle's on the two-symbol frame), else
    on the unscaled samples (the oracle's on the frame times a power of two that needs no
    rescaling; the estimate is invariant under it)."""
    two = np.asarray(row[:2 * (1 << sf) * osr], np.complex64)
    if not (sf <= 9 and osr == 1):
        m = float(np.abs(two.view(np.float32)).max())
        if m > 1.0:
            two = (two * np.float32(2.0 ** -int(np.ceil(np.log2(m))))).astype(np.complex64)
    return t_off_of(O.lora_demodulate(two, sf, osr, hann)[3])


def offset_frames(O, sf, osr, F, snr_db, seed, hann=False, split=True):
    """Family (b), real offsets, as RAW input: oracle-modulated frames of 37 random symbols at
    amplitude 2.5 with a carrier offset near 0.3 bin and a delay of +-3 samples (drate != 0 and
    t_off != 0 in the bound), noiseless (snr_db None) or with noise.  The last frame's symbol 0 is
    two equal-power bins an odd distance apart in the dechirped domain: which one the estimate
    picks is a matter of rounding, and picking the other moves the time offset by N/2.  For the
    noiseless family (`split`) the second tone's phase is searched, on the oracle, for one where
    the pre-pass estimate (prepass_t_off) and the exact one disagree, so that a LEGACY frame
    whose every symbol must be recomputed is part of the batch; one of its data symbols is 1.2
    times as large, so that the frame's maximum is not the sync windows'."""
    N = 1 << sf
    step = N * osr
    L = S_TOTAL * step
    rng = np.random.default_rng(seed)
    up = np.conj(down_chirp(O, sf, osr))
    out = np.zeros((F, L), np.complex64)
    n = np.arange(L)
    for f in range(F):
        syms = rng.integers(0, N, S_TOTAL - 2).astype(np.uint16)
        x = O.lora_modulate(syms, sf, osr, 125000, 1.0, 0x12).astype(np.complex128)[:L]
        x = x * np.exp(2j * np.pi * (0.3 + 0.02 * f) * n / step)
        d = 3 * osr
        x = np.concatenate([np.zeros(d), x])[:L] if f % 2 == 0 else np.concatenate([x[d:], np.zeros(d)])
        x = 2.5 * x
        if snr_db is not None:
            sigma = 2.5 * 10 ** (-snr_db / 20) / np.sqrt(2)
            x = x + sigma * (rng.standard_normal(L) + 1j * rng.standard_normal(L))
        if f == F - 1:
            x[5 * step:6 * step] *= 1.2  # a data window above the sync windows: k_est_split's scale guess fails
            for j in range(64 if (split and snr_db is None) else 1):
                tie = tone(step, 10, N, osr, 1.375) + tone(step, 41, N, osr, 1.375, 0.3 + 0.37 * j)
                x[:step] = tie * up
                row = O.dechirp(x.astype(np.complex64), sf, osr)
                if prepass_t_off(O, row, sf, osr, hann) != t_off_of(O.lora_demodulate(row, sf, osr, hann)[3]):
                    break
        out[f] = x.astype(np.complex64)
    return out


def plan_input(O, raw, sf, osr, mode, dechirp):
    """What the plan of a variant is fed for the RAW-input frames `raw`: themselves when it
    dechirps (fused legacy / raw, and api), else the oracle's dechirped frames."""
    if mode == "api" or dechirp:
        return raw
    return np.stack([O.dechirp(r, sf, osr) for r in raw])


def oracle_frame(O, row, sf, osr, mode, dechirp, hann):
    """(symbols, sync, cfo, time_offset) of one plan-input frame by the CPU oracle."""
    if mode == "api":
        r, syms, sync, cfo, toff = O.api_demodulate(row, sf, osr, hann)
        assert r == len(row) // ((1 << sf) * osr) - 2
        return syms, sync, cfo, toff
    if mode == "raw":
        return O.raw_demod(row, sf, osr, hann, dechirp=dechirp), 0, 0.0, 0.0
    return O.lora_demodulate(O.dechirp(row, sf, osr) if dechirp else row, sf, osr, hann)


def rate_of(cfo, sf):
    """FrameParams.rate from the cfo output, in the kernels' fp32 operations."""
    return np.float32(np.float32(np.float32(-2.0) * np.float32(np.pi)) * np.float32(cfo)) / np.float32(1 << sf)


# ---- the reference's share of the bound ---------------------------------------------------

def share_windows(sf, rng):
    """Gaussian windows at amplitudes 1e-3 .. 3e4 and near-tie two-tone windows of N points."""
    N = 1 << sf
    out = [(a * (rng.standard_normal(N) + 1j * rng.standard_normal(N))).astype(np.complex64)
           for a in (1e-3, 0.01, 0.3, 1.0, 3.0, 100.0, 3e4) for _ in range(3)]
    out += [(tone(N, 5, N, 1, 1.3) + tone(N, N // 2 + 9, N, 1, 1.3 * (1.0 + d), 0.7)).astype(np.complex64)
            for d in DELTAS[::2] + DELTAS[1::6]]
    return out


def reference_share(O, sf, hann, seed=40):
    """Worst |X32_k - X64_k| / (E sum|y_i|) over share_windows: the oracle's fp32 transform
    (with the fp32 Hann product when `hann`) against the float64 one, in units of E = (8 SF +
    42) 2^-24 - the share of the bound DESIGN.md §3.4 grants each path's transform."""
    E = (8.0 * sf + 42.0) * U
    w = hann_table(1 << sf) if hann else None
    worst = 0.0
    for y in share_windows(sf, np.random.default_rng(seed + sf)):
        z32 = (y * w).astype(np.complex64) if hann else y  # complex64 x float32: one rounding per component
        err = np.abs(O.fft(z32).astype(np.complex128) - spectrum_f64(y, 0.0, w)).max()
        worst = max(worst, float(err / np.abs(y.astype(np.complex128)).sum()) / E)
    return worst


# ---- the kernels against the model --------------------------------------------------------

def f32(bits):
    return float(np.uint32(bits).view(np.float32))


def evaluate(O, variant, x, symbols, tr, deltas=None):
    """Hold one run to the model.  x: the plan's input [F, L]; symbols: its [F, S] output; tr:
    ``DemodPlan.spec_trace()`` of that run; deltas: the sweep's [F, 37] (family a) or None.
    Returns a dict of findings, every list empty when the kernels agree with the model:
      wmax_bad      (f, s, got, want): a data window's recorded maximum is not window_max's bits
      slot_bad      (f, got, want): the frame's slot is not slot_max's bits (LEGACY)
      expected      the set of (f, s | SYNC_PAIR) `certified` rejects on the GPU's own record
      listed        the reject list as [(f, s)]
      over          (f, s, err, allowed): |recorded margin - margin_f64| > 2 n1 (e_spec + E)
      argmax_bad    (f, s, float64 argmax, got): a certified symbol is not the float64 argmax
      edge_missing  (f, s, delta): a sweep symbol with |delta| <= 2^-20 is not on the list
      wide_listed   (f, s, d64, B): a symbol whose float64 margin exceeds 8 B is on the list
      t_split       frames whose exact and speculative t_off differ
      worst         the largest |margin error| / (n1 (e_spec + E)) seen."""
    mode, sf, osr, window, dechirp = variant
    N = 1 << sf
    F, L = x.shape
    total = L // (N * osr)
    w = hann_table(N) if window == "hann" else None
    s0 = 0 if mode == "raw" else 2
    listed = [(int(f), int(s)) for f, s in tr.rejected]
    lset = set(listed)
    rep = dict(wmax_bad=[], slot_bad=[], expected=set(), listed=listed, over=[], argmax_bad=[], edge_missing=[],
               wide_listed=[], t_split=[], worst=0.0)
    for f in range(F):
        fp, fps = tr.fp[f], tr.fp_spec[f]
        same_t = int(fp["t_off"]) == int(fps["t_off"])
        if not same_t:
            rep["t_split"].append(f)
        wins = windows(O, x[f], sf, osr, mode, dechirp, int(fps["t_off"]))
        E, e_spec, _, _, _ = bound_terms(sf, fp["rate"], fps["rate"], fp["t_off"])
        rate = float(fps["rate"])
        sync_ok = True
        for s in range(total):
            if s < s0:
                if mode == "api":
                    continue  # the estimate kernel demodulated the sync symbols exactly
                wmax = f32(tr.max_slot[f])
            else:
                want = window_max(wins[s])
                if want != int(tr.aux[f, s]):
                    rep["wmax_bad"].append((f, s, int(tr.aux[f, s]), want))
                wmax = f32(tr.aux[f, s])
            d = float(tr.margin[f, s])
            d64, k64 = margin_f64(wins[s][::osr], rate, w)
            unit = 2.0 * N * wmax * (e_spec + E)
            err = abs(d - d64)
            if err > 2.0 * unit:
                rep["over"].append((f, s, err, 2.0 * unit))
            rep["worst"] = max(rep["worst"], err / unit if unit > 0 else (0.0 if err == 0 else np.inf))
            ok = certified(tr.margin[f, s], wmax, s, fp, fps, sf, mode)
            if s < s0:
                sync_ok = sync_ok and ok
                if ok and k64 != int(tr.aux[f, s]):
                    rep["argmax_bad"].append((f, s, k64, int(tr.aux[f, s])))
                continue
            if not ok:
                rep["expected"].add((f, s))
            elif k64 != int(symbols[f, s - s0]):
                rep["argmax_bad"].append((f, s, k64, int(symbols[f, s - s0])))
            B = bound(wmax, s, sf, fp["rate"], fps["rate"], fp["t_off"])
            if same_t and d64 > 8.0 * B + 2.0 ** -60 and (f, s) in lset:
                rep["wide_listed"].append((f, s, d64, B))
            if deltas is not None and s >= 2 and abs(deltas[f, s - 2]) <= 2.0 ** -20 and (f, s) not in lset:
                rep["edge_missing"].append((f, s, float(deltas[f, s - 2])))
        if mode == "legacy":
            if not sync_ok:
                rep["expected"].add((f, SYNC_PAIR))
            want = slot_max(O, x[f], sf, osr, dechirp, int(fps["t_off"]))
            if want != int(tr.max_slot[f]):
                rep["slot_bad"].append((f, int(tr.max_slot[f]), want))
    return rep


FAMILIES = ("sweep", "sweep_small", "offsets", "offsets_noisy")


def family_frames(O, variant, family):
    """(plan input [F, L], deltas or None) of one input family for a variant."""
    mode, sf, osr, window, dechirp = variant
    F = frames_of(sf)
    deltas = None
    if family.startswith("sweep"):
        raw, deltas = sweep_frames(O, sf, osr, F, 1.0 if family == "sweep" else 0.4 / 1.7, chirped_sync=mode != "api")
    else:
        raw = offset_frames(O, sf, osr, F, None if family == "offsets" else -10.0, 6100 + 10 * sf + osr,
                            hann=window == "hann", split=mode == "legacy")
    return plan_input(O, raw, sf, osr, mode, dechirp), deltas
