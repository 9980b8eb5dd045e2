/*
 * lora_mi355x.h — C-ABI of the MI355X LoRa PHY demodulator/modulator.
 *
 * This is the drop-in boundary for the reference's hot path.  Every entry point
 * names the reference interface it replaces (paths relative to the reference
 * checkout yakir1991/LoRa-SDR-Lightweight-Standalone-Library-):
 *
 *   lora_demod_plan_create / _destroy
 *       replaces lora_phy::lora_demod_init / lora_demod_free
 *       (include/lora_phy/phy.hpp:190-194, src/phy/LoRaDemod.cpp:10-47) and, in
 *       LORA_MODE_API, lora_phy::init (phy.hpp:102, phy.cpp:26-49).
 *   lora_demod_batch
 *       replaces lora_phy::lora_demodulate (phy.hpp:204-207, LoRaDemod.cpp:49-195),
 *       one call per frame in the reference, F frames per call here; with
 *       params.dechirp = 1 it also absorbs the caller-side dechirp loop every
 *       reference caller runs first (tests/e2e_chain_test.cpp:85-93).
 *       In LORA_MODE_API it replaces lora_phy::demodulate (phy.hpp:134-136,
 *       phy.cpp:178-239) including estimate_offsets (phy.cpp:78-145) and
 *       get_last_metrics (phy.cpp:258-261).
 *   lora_mod_batch
 *       replaces lora_phy::lora_modulate (phy.hpp:198-201, LoRaMod.cpp:8-43) and
 *       lora_phy::modulate (phy.hpp:126-128, phy.cpp:65-76).
 *
 * Conventions: plain pointers and sizes only.  IQ buffers are interleaved fp32
 * (I,Q) pairs — the layout of std::complex<float> and torch.complex64 — and live in
 * device memory (HBM) of the plan's device.  The caller owns every buffer
 * (API_SPEC.md ownership rule); the plan owns only its constant tables.  No call
 * allocates or synchronises: `stream` is a hipStream_t (NULL = default stream); the
 * work is enqueued on it and nothing else, so the calls are hipGraph-capturable.
 * A plan may be used by one host thread at a time.
 *
 * Errors are negative errno values (the reference returns -1, phy.cpp:27,58,181-190);
 * lora_last_error() gives a thread-local message.
 */
#ifndef LORA_MI355X_H
#define LORA_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LORA_OK 0
#define LORA_EIO (-5)     /* HIP runtime error */
#define LORA_ENOMEM (-12) /* device allocation failed at plan creation */
#define LORA_EINVAL (-22) /* bad parameter / size (reference: -1) */
#define LORA_ERANGE (-34) /* output capacity too small (reference: -1) */

/* phy.hpp:29-32 */
#define LORA_WINDOW_NONE 0
#define LORA_WINDOW_HANN 1

/* LEGACY: lora_demodulate semantics (LoRaDemod.cpp:49-195): max-amplitude
 *   normalisation, 2-symbol CFO/timing estimate on the (dechirped) input, per-symbol
 *   CFO rotation + FFT + argmax; frames of any length, sync nibbles from symbols 0/1.
 * API: lora_phy::demodulate semantics (phy.cpp:178-239): no normalisation, estimate
 *   on the raw input, per-symbol fused down-chirp; frame length must be a whole
 *   number (>= 2) of symbols. */
#define LORA_MODE_LEGACY 0
#define LORA_MODE_API 1
/* RAW: the detector primitive alone - per whole symbol: (dechirp) -> (window) ->
 *   2^SF FFT -> lowest-index argmax |X|^2 (LoRaDetector.hpp:39-58), no normalisation,
 *   no offset estimate, no rotation, every symbol output (no sync word: sync, cfo,
 *   time_offset, max_amp are written as 0).  This is the demodulator of the
 *   reference's Python AWGN sweep (tests/awgn_sweep.py:262-265). */
#define LORA_MODE_RAW 2

/* Rotation arithmetic of the symbol demod (lora_demod_batch, LEGACY / API modes).
 * EXACT: bit-identical to the reference (glibc sincosf per sample, LoRaDemod.cpp:151-157;
 *   every output equals lora_demodulate's).  The default.
 * FAST: the per-sample CFO rotation uses the hardware sine/cosine (v_sin/v_cos_f32 on
 *   the phase in revolutions, absolute phase error ~1e-5 rad) instead of glibc's
 *   double-precision polynomial.  The normalisation, the offset estimate (cfo,
 *   time_offset) and the sync word stay exact; data symbol indices equal the reference
 *   except where two FFT bins are within rounding of each other (near-ties under
 *   noise).  Stated tolerance, checked by tests/test_gpu_fast_rotation.py: identical
 *   symbols on noiseless and >= 0 dB frames; >= 99 % per-symbol agreement at -10 dB
 *   SF7, and SER within 0.01 absolute of the exact path at any SNR. */
#define LORA_PRECISION_EXACT 0
#define LORA_PRECISION_FAST 1

typedef struct lora_demod_plan lora_demod_plan;

typedef struct {
  unsigned sf;    /* spreading factor, 2..12 (N = 2^sf <= 4096, kissfft.hh:34) */
  unsigned osr;   /* oversampling ratio >= 1 (0 is treated as 1, phy.cpp:32) */
  unsigned bw_hz; /* 125000, 250000 or 500000 (phy.hpp:37-41) */
  int window;     /* LORA_WINDOW_* */
  int dechirp;    /* LEGACY / RAW: 1 = input is raw IQ, multiply sample j of each frame
                     by genChirp(N, osr, N*osr, down)[j mod N*osr] first
                     (e2e_chain_test.cpp:85-93); 0 = input already dechirped */
  int mode;       /* LORA_MODE_* */
  int device;     /* HIP device ordinal */
  int precision;  /* LORA_PRECISION_* (0 = EXACT) */
} lora_demod_params;

/* Per-frame outputs; any pointer may be NULL.  Device pointers. */
typedef struct {
  uint16_t* symbols;     /* [frames][sym_stride]; symbol indices (LoRaDemod.cpp:165-174) */
  int64_t sym_stride;    /* elements between frames in `symbols` (>= symbols per frame) */
  uint8_t* sync;         /* [frames] sync word from symbols 0/1 (LoRaDemod.cpp:177-192) */
  float* cfo;            /* [frames] lora_metrics.cfo (LoRaDemod.cpp:131) */
  float* time_offset;    /* [frames] lora_metrics.time_offset (LoRaDemod.cpp:134-135) */
  float* max_amp;        /* [frames] LEGACY: max(|I|,|Q|) of the (dechirped) frame
                            (LoRaDemod.cpp:59-67); callers emulating the scratch-size
                            rule (LoRaDemod.cpp:69-71) need it */
} lora_demod_outputs;

int lora_demod_plan_create(const lora_demod_params* params, lora_demod_plan** plan);
int lora_demod_plan_destroy(lora_demod_plan* plan);

/* Symbols each frame of `frame_len` samples yields (>= 0), or a negative error
 * (LORA_MODE_API: frame_len must be a multiple of N*osr with >= 2 symbols). */
int64_t lora_demod_symbols_per_frame(const lora_demod_plan* plan, int64_t frame_len);

/* Device workspace bytes lora_demod_batch needs for `frames` frames of `frame_len`
 * samples (0 when frames is 0).  The reference's workspace is caller-owned too
 * (lora_demod_workspace, phy.hpp:170-185, plus its scratch buffer sized to the frame). */
size_t lora_demod_workspace_bytes(const lora_demod_plan* plan, int64_t frames, int64_t frame_len);

/* Demodulate `frames` frames of `frame_len` complex samples each, frame f starting
 * at iq + 2*f*frame_stride floats.  `workspace` must hold
 * lora_demod_workspace_bytes(plan, frames, frame_len) bytes of device memory (may be NULL
 * if 0).
 * Returns symbols per frame (>= 0) or a negative error. */
int64_t lora_demod_batch(lora_demod_plan* plan, const float* iq, int64_t frames,
                         int64_t frame_len, int64_t frame_stride, const lora_demod_outputs* out,
                         void* workspace, size_t workspace_bytes, void* stream);

/* lora_phy::estimate_offsets (phy.hpp:142-144, phy.cpp:78-145) for F frames: every
 * whole symbol of each frame, osr phases, raw (not dechirped, not normalised)
 * windowed samples, plain '>' phase selection.  Writes cfo[f] / time_offset[f]
 * (device arrays) unless the frame holds no whole symbol, in which case the
 * outputs are left untouched (phy.cpp:81,87).  Uses the plan's sf/osr/window only.
 * Returns the number of symbols each frame's estimate used. */
int64_t lora_estimate_offsets_batch(lora_demod_plan* plan, const float* iq, int64_t frames,
                                    int64_t frame_len, int64_t frame_stride, float* cfo,
                                    float* time_offset, void* stream);

/* lora_phy::compensate_offsets (phy.hpp:150-152, phy.cpp:147-176) for F frames,
 * out of place: out[f] = shift(in[f] * exp(j*rate*n)), rate = -2*pi*cfo[f]/(N*osr),
 * shift by round(time_offset[f]) samples with zero fill.  `in` and `out` must not
 * overlap (the caller copies back for the reference's in-place semantics).
 * cfo / time_offset are device arrays of `frames` floats.  Returns frame_len. */
int64_t lora_compensate_offsets_batch(unsigned sf, unsigned osr, const float* in, int64_t frames,
                                      int64_t frame_len, int64_t frame_stride, const float* cfo,
                                      const float* time_offset, int device, void* stream,
                                      float* out);

/* Per-symbol detector metrics: what LoRaDetector<float>::detect returns beside the index
 * (LoRaDetector.hpp:39-74), which every reference caller receives (LoRaDemod.cpp:99-100,
 * 163-164, phy.cpp:111-112,226-227) and lora_demod_batch drops.  Rows are `stride` elements
 * apart; column s is whole symbol s of the frame, 0 <= s < total = frame_len / (N*osr): the
 * sync symbols are columns 0 and 1 (no offset by 2 as in lora_demod_outputs.symbols).
 * Device pointers; any pointer may be NULL. */
typedef struct {
  float* power;      /* [frames][stride] detect()'s power, dB   (LoRaDetector.hpp:64) */
  float* power_avg;  /* [frames][stride] detect()'s powerAvg    (LoRaDetector.hpp:60-63) */
  float* f_index;    /* [frames][stride] detect()'s fIndex      (LoRaDetector.hpp:66-71) */
  uint16_t* index;   /* [frames][stride] detect()'s return value (LoRaDetector.hpp:73) */
  int64_t stride;    /* elements between frames, >= symbols per frame */
} lora_symbol_metrics;

/* The detector's outputs for every whole symbol of `frames` frames laid out as for
 * lora_demod_batch, on the FFT input the reference feeds for that symbol in the plan's mode:
 *   LEGACY (LoRaDemod.cpp:137-164): t_off = (int)round(time_offset[f]), rate =
 *     -2*pi*cfo[f]/N, the window base with the guards of :143-149, then per point the
 *     caller-side dechirp (params.dechirp), the scale 1/max_amp[f] when max_amp[f] > 1
 *     (:68-77), the cosf/sinf rotation (:151-158) and the window (:159-160);
 *   API (phy.cpp:197-227): a fresh down-chirp's [i] per symbol, the same rotation and base
 *     rule, no normalisation (max_amp is ignored and may be NULL);
 *   RAW: (dechirp) -> window -> detect; cfo, time_offset and max_amp are ignored and may be
 *     NULL.
 * cfo / time_offset / max_amp are device arrays of `frames` floats: the values
 * lora_demod_batch wrote for the same frames.  Any float is accepted: the conversion of
 * time_offset saturates (NaN gives 0) and the base guards keep every window in its frame.
 * The arithmetic is always the exact one (bit-identical to detect(), including the double
 * total taken in bin order, :45-52), whatever precision and pipeline the plan was made with.
 * Enqueues one kernel on `stream`, allocates and synchronises nothing, needs no workspace,
 * and fully writes columns 0 .. total-1 of every output given and nothing beyond them.
 * frames == 0, total == 0 or all four outputs NULL: no launch.  LORA_EINVAL, before any HIP
 * call: a NULL plan, out or iq (frames > 0), negative sizes, frame_len >= 2^31, frame_stride <
 * frame_len with more than one frame, stride < total with an output given, a NULL cfo /
 * time_offset / max_amp in LEGACY, a NULL cfo / time_offset in API; in API mode frame_len
 * must satisfy lora_demod_symbols_per_frame (phy.cpp:186-188).  Returns total. */
int64_t lora_demod_metrics_batch(lora_demod_plan* plan, const float* iq, int64_t frames,
                                 int64_t frame_len, int64_t frame_stride, const float* cfo,
                                 const float* time_offset, const float* max_amp,
                                 const lora_symbol_metrics* out, void* stream);

/* Soft bits per symbol: a max-log LLR for each of the sf bits a symbol carries, from the same
 * spectrum lora_demod_metrics_batch reduces to one index.  Frames, cfo / time_offset / max_amp
 * and the FFT input of every whole symbol are exactly those of lora_demod_metrics_batch
 * (LoRaDemod.cpp:137-164, phy.cpp:197-227, or the bare detector in LORA_MODE_RAW), with the
 * exact arithmetic whatever precision and pipeline the plan was made with.  Column s is whole
 * symbol s, 0 <= s < total = frame_len / (N*osr); the sync symbols are columns 0 and 1.
 * llr is [frames][llr_stride][sf] floats, llr_stride in symbols: bit c of symbol s of frame f
 * is llr[(f * llr_stride + s) * sf + c].  For one symbol with spectrum X:
 *   P[k] = re*re + im*im in fp32, no contraction (LoRaDetector.hpp:51);
 *   Q[k] = P[k] > 0 ? P[k] : 0 (the detector's strict '>', :53-57: NaN and 0 never win);
 *   v(k) = grayToBinary16(k), the value the chain deinterleaves (LoRaCodes.hpp:212-222);
 *   m1 = max{Q[k] : bit c of v(k) = 1}, m0 = max{Q[k] : bit c of v(k) = 0};
 *   llr[c] = (m1 == m0) ? +0.0f : m1 - m0, one fp32 subtraction.
 * Positive means the bit is 1; wherever llr[c] != 0 its sign is bit c of grayToBinary16 of the
 * detector's index.  A silent window and inf - inf give +0.0f, so no NaN is ever written.  The
 * values are not normalised by the noise floor (lora_decode_chain_soft_batch is scale-free;
 * power_avg of lora_demod_metrics_batch is the floor).  The detector's double total is not
 * computed.  This definition is the library's own: the reference has no soft path.
 * Enqueues one kernel on `stream`, allocates and synchronises nothing, needs no workspace, and
 * fully writes columns 0 .. total-1 of every row and nothing beyond them.  frames == 0,
 * total == 0 or a NULL llr: no launch.  LORA_EINVAL, before any HIP call: everything
 * lora_demod_metrics_batch refuses, llr_stride < total, and a plan with sf < 6 (the chain that
 * consumes the bits is defined for SF 6-12).  Returns total. */
int64_t lora_demod_soft_bits_batch(lora_demod_plan* plan, const float* iq, int64_t frames,
                                   int64_t frame_len, int64_t frame_stride, const float* cfo,
                                   const float* time_offset, const float* max_amp,
                                   float* llr, int64_t llr_stride, void* stream);

/* lora_demod_soft_bits_batch for self-describing frames ("Self-describing frames", below):
 * columns red_first .. red_first + red_count - 1 of every frame are REDUCED, the others are
 * exactly lora_demod_soft_bits_batch's.  A reduced column is a symbol of a frame's header block,
 * which carries sf - 2 bits in multiples of four bins and is rounded to the nearest one
 * (r = ((s + 2) >> 2) & (2^(sf-2) - 1), then grayToBinary16, LoRaCodes.hpp:212-222).  With Q as
 * above:
 *   v'(k) = grayToBinary16(((k + 2) >> 2) & (2^(sf-2) - 1));
 *   for c < sf - 2: m1 = max{Q[k] : bit c of v'(k) = 1}, m0 = max{Q[k] : bit c of v'(k) = 0},
 *     llr[c] = (m1 == m0) ? +0.0f : m1 - m0;
 *   llr[sf-2] = llr[sf-1] = +0.0f.
 * (Bit c of v'(k) is bit c + 2 of grayToBinary16((k + 2) mod N): a reduced column is bits
 * 2 .. sf-1 of the spectrum rotated by two bins.)  Maxima are exact in any order, so the values
 * are reproducible to the bit, as the full-rate ones.  With the sync symbols in columns 0 and 1
 * of a LEGACY / API frame its header is columns 2 .. 9: red_first = 2, red_count = 8.
 * LORA_EINVAL, before any HIP call: everything lora_demod_soft_bits_batch refuses, a negative
 * red_first or red_count, red_first + red_count > total, and red_count > 0 on a plan with
 * sf < 7.  red_count == 0 is lora_demod_soft_bits_batch itself, bit for bit.  Returns total. */
int64_t lora_demod_soft_bits_frame_batch(lora_demod_plan* plan, const float* iq, int64_t frames,
                                         int64_t frame_len, int64_t frame_stride, const float* cfo,
                                         const float* time_offset, const float* max_amp,
                                         float* llr, int64_t llr_stride, int64_t red_first,
                                         int64_t red_count, void* stream);

/* Sliding detector scan of continuous streams: LoRaDetector<float>::detect
 * (LoRaDetector.hpp:39-74) on a window of step = N*osr samples that starts every `hop` samples
 * of each of `rows` rows of `row_len` complex samples (row r at iq + 2*r*row_stride floats).
 * Window w of a row starts at sample w*hop; a row has
 *   W = row_len < step ? 0 : (row_len - step) / hop + 1
 * of them and none reads past row_len.  The FFT input of a window is what a LORA_MODE_RAW plan
 * feeds for a one-symbol frame cut at that sample: point i is x[w*hop + i*osr], times
 * down[i*osr] (the table index counts from the window start) when params.dechirp is set, times
 * the window table for LORA_WINDOW_HANN; no normalisation, estimate or rotation.  Every output
 * is bit-identical to what lora_demod_metrics_batch returns in LORA_MODE_RAW for the same
 * N*osr samples given as one frame (the exact arithmetic, including the double total taken in
 * bin order, LoRaDetector.hpp:45-52).  The outputs are lora_symbol_metrics' four, laid out
 * [rows][stride] with column w.  Uses the plan's sf, osr, bw, window and dechirp only; the mode
 * is ignored, as in lora_estimate_offsets_batch.  Any hop >= 1 is legal (odd, or > step).
 *
 * lora_detect_scan_windows: host arithmetic only; W, or LORA_EINVAL for a NULL plan, a
 * negative row_len or hop < 1.
 * lora_detect_scan_batch: enqueues one kernel on `stream`, allocates and synchronises nothing,
 * needs no workspace, and fully writes columns 0 .. W-1 of every output given and nothing
 * beyond them.  rows == 0, W == 0 or all four outputs NULL: no launch.  LORA_EINVAL, before
 * any HIP call: a NULL plan or out, a NULL iq with work to do, negative sizes, hop < 1,
 * row_len >= 2^31, row_stride < row_len with more than one row, out->stride < W with an
 * output given, a grid beyond 2^31 (rows * ceil(W / windows per workgroup)).  Returns W. */
int64_t lora_detect_scan_windows(const lora_demod_plan* plan, int64_t row_len, int64_t hop);
int64_t lora_detect_scan_batch(lora_demod_plan* plan, const float* iq, int64_t rows, int64_t row_len,
                               int64_t row_stride, int64_t hop, const lora_symbol_metrics* out, void* stream);

/* The frame finder on the device: frame starts from the scan's outputs, by the rule that
 * lora_phy_amd/stream.py states (the reference has no frame detector; the rule is the library's
 * own).  The inputs are three of lora_detect_scan_batch's outputs for `rows` rows of W windows,
 * made with this hop by a dechirping plan of this sf and osr at bw 125 kHz (the entry knows no
 * bandwidth and cannot check it): power, power_avg and index, laid out [rows][stride] with
 * column w.  With N = 2^sf, step = N*osr, k = step / hop, sw0 = (sync >> 4) << (sf - 4),
 * sw1 = (sync & 15) << (sf - 4) (sync taken mod 256), frame_len = (frame_symbols + 2) * step:
 *   snr[w] = power[w] - power_avg[w], one fp32 subtraction, and ok[w] = snr[w] >= thresh_db in
 *     fp32: NaN fails, +inf passes;
 *   window w, 0 <= w < W - k, is a candidate when ok[w], ok[w + k] and
 *     (index[w + k] - index[w]) mod N == (sw1 - sw0) mod N;
 *   d = (index[w] - sw0) mod N, minus N when d >= N/2, and start = w*hop - d*osr in int64;
 *   the greedy pass runs in increasing w from ceil(max(first - step/2, 0) / hop): a candidate
 *     with start >= first, start >= 0 and start + frame_len <= row_len is accepted, first becomes
 *     start + frame_len and the pass continues at the smallest w' > w with w'*hop >= first -
 *     step/2; anything else moves on to w + 1.
 * `first` is a device array of one int64 per row, or NULL for 0 in every row.  Per row:
 *   count   the frames the pass accepts; the pass does not depend on capacity, so count may
 *           exceed it;
 *   starts  [rows][capacity]: the first min(count, capacity) accepted starts, increasing, then
 *           -1 in every further slot;
 *   end     first as the pass leaves it: the end of the last accepted frame, or the first given
 *           when none was accepted - what a chunked caller carries into its next chunk.
 * All three equal the rule applied on the host, as integers.
 *
 * lora_find_frames_batch: enqueues one kernel on `stream` of params.device, allocates and
 * synchronises nothing, needs no workspace, and fully writes count, end and all `capacity` slots
 * of starts for every row - also for rows with W <= k (count 0, end = first) and for capacity 0.
 * One workgroup per row; no workgroup waits on another.  rows == 0: no launch.  LORA_EINVAL,
 * before any HIP call: a NULL params, a NULL count or end, a NULL starts with capacity > 0 or
 * NULL metrics with W > k (each with rows > 0), sf outside 6..12, osr outside 1..65536, hop < 1,
 * hop not dividing step or step / hop < 2, frame_symbols outside 0 .. 2^31 - 1, negative rows,
 * W, stride, row_len or capacity, stride < W with more than one row, W >= 2^31, rows >= 2^31.
 * Returns rows.
 * lora_find_frames_tile: the windows per tile of the kernel's pass (its state crosses a tile
 * boundary every so many windows); host arithmetic only. */
typedef struct {
  unsigned sf;
  unsigned osr;
  unsigned sync;
  float thresh_db;
  int64_t hop;
  int64_t frame_symbols;
  int device;
} lora_find_params;
int64_t lora_find_frames_tile(void);
int64_t lora_find_frames_batch(const lora_find_params* params, const float* power, const float* power_avg,
                               const uint16_t* index, int64_t rows, int64_t W, int64_t stride,
                               const int64_t* first, int64_t row_len, int64_t capacity, int64_t* starts,
                               int32_t* count, int64_t* end, void* stream);

/* The finder for frames that state their own length ("Self-describing frames", below): the
 * candidates are listed, a caller decodes the header at each (lora_gather_frames_batch,
 * lora_demod_batch, lora_decode_frame_batch in header-only mode), and the greedy pass runs over
 * the slots whose header is good, each frame as long as its header says.  Like the finder above
 * the rule is the library's own.
 *
 * lora_find_candidates_batch: the candidate rule and the refinement of lora_find_frames_batch,
 * unchanged (same inputs, same fp32 comparison; params.frame_symbols is not used).  Per row, in
 * increasing w, a candidate's start is listed when start >= 0 and start + 10 * step <= row_len
 * (the two sync symbols and the header's eight fit), unless it equals the row's last listed
 * start.  count[r] = the starts listed (may exceed capacity), starts [rows][capacity] = the first
 * min(count, capacity) of them, then -1.
 * lora_select_frames_batch: per row, `slots` candidate slots - cand_starts, and status and nsym
 * as lora_decode_frame_batch gave them for each, all [rows][slots].  In slot order, slot j is
 * accepted when status is LORA_FRAME_OK, nsym <= max_symbols, start >= first (and >= 0: an
 * empty slot is -1) and start + (2 + nsym) * step <= row_len; first then becomes that end.
 * (The fixed-length pass's jump to first - step/2 needs no restating: |d * osr| <= step/2.)
 * count, starts and end as lora_find_frames_batch's, and nsym [rows][capacity], 0 in the empty
 * slots.  `first`: one int64 per row on the device, or NULL for 0.
 * Both: one kernel on `stream`, one workgroup per row, nothing allocated or synchronised, every
 * output fully written (also with no window to test, no slot, or capacity 0); rows == 0: no
 * launch.  LORA_EINVAL before any HIP call as for lora_find_frames_batch, and for step < 1,
 * max_symbols < 0 or slots >= 2^31.  Return rows. */
int64_t lora_find_candidates_batch(const lora_find_params* params, const float* power, const float* power_avg,
                                   const uint16_t* index, int64_t rows, int64_t W, int64_t stride,
                                   int64_t row_len, int64_t capacity, int64_t* starts, int32_t* count,
                                   void* stream);
int64_t lora_select_frames_batch(const int64_t* cand_starts, const int32_t* status, const int32_t* nsym,
                                 int64_t rows, int64_t slots, const int64_t* first, int64_t row_len, int64_t step,
                                 int64_t max_symbols, int64_t capacity, int64_t* starts, int32_t* out_nsym,
                                 int32_t* count, int64_t* end, int device, void* stream);

/* Preambled frames: a preamble and a start-of-frame delimiter (SFD) in front of the frame, so
 * that a receiver can sum spectra over symbols and tell a carrier offset from a timing offset.
 * The layout is the library's own (no interoperability with a radio is claimed).  With N = 2^sf,
 * step = N*osr and genChirp as ChirpGenerator.hpp:23-50, a preambled frame of P preamble
 * symbols and S data symbols is four parts, each from its own genChirp chain that starts at
 * phase 0, with the amplitude clamped to [-1, 1] as lora_mod_batch clamps it (LoRaMod.cpp:16):
 *   pre    P up-chirps genChirp(f0 = 0, NN = step, down = false), phase carried from one to the
 *          next; P is 4..64;
 *   sync   the two sync symbols exactly as lora_mod_batch emits them: samples [0, 2*step) of its
 *          frame;
 *   sfd    two down-chirps genChirp(f0 = 0, NN = step, down = true) and a quarter of one
 *          (NN = step/4), phase carried;
 *   data   the data symbols exactly as lora_mod_batch emits them: samples [2*step, (2+S)*step)
 *          of the same frame.
 * The length is (P + 2 + S)*step + tail, tail = 9*step/4.  The phase is NOT continuous across the
 * three joins, on purpose: a receiver that gathers [sync | data] has lora_mod_batch's frame bit
 * for bit, so every bit-exact contract of the demodulator, the header and the CRC carries over,
 * and the receiver is non-coherent across symbols anyway.  (A phase-continuous modulator kernel
 * is not provided.)  "start" of a preambled frame is the sample of its first sync symbol, as
 * everywhere else.
 *
 * lora_preamble_tables: host arithmetic only (no HIP call): writes pre (P*step complex samples,
 * 2 floats each) and sfd (tail samples) into host buffers; either may be NULL.  Returns P*step.
 * LORA_EINVAL: sf outside 2..12, a bad bw_hz, preamble outside 4..64, step not a multiple of 4.
 * osr 0 is taken as 1. */
int64_t lora_preamble_tables(unsigned sf, unsigned osr, unsigned bw_hz, float amplitude, int64_t preamble,
                             float* pre, float* sfd);

/* The accumulating scan: lora_detect_scan_batch's spectra summed over `acc` consecutive symbols.
 * W is lora_detect_scan_windows' count and k = step / hop.  acc is 1..8; with acc > 1 hop must
 * divide step.  Wa = W - (acc-1)*k when that is positive, else 0.  Window w of the plain scan
 * has the spectrum P_w[b] = re*re + im*im of lora_detect_scan_batch's FFT (same loads, dechirp
 * product, window and transform, no contraction); with conj != 0 every sample is conjugated
 * before the dechirp product, so the entry equals the scan of the conjugated stream (a
 * down-chirp then dechirps like an up-chirp).  The summed spectrum is
 *   S_w[b] = (((P_w[b] + P_{w+k}[b]) + P_{w+2k}[b]) + ...)   acc terms, fp32, in this order,
 * one rounding per addition, summed afresh for every w.  For w < Wa:
 *   index      the lowest-index maximum of S_w, strict '>' from 0 (LoRaDetector.hpp:53-57);
 *   power      20*log10f(sqrtf(maxv)) - power_scale, maxv the maximum (LoRaDetector.hpp:61,64);
 *   power_avg  20*log10f(sqrtf((float)(total - maxv))) - power_scale, total the double sum of S_w
 *              in bin order (LoRaDetector.hpp:39-74's statements on S_w).
 * There is no f_index.  acc == 1 with conj == 0 equals lora_detect_scan_batch bit for bit.  The
 * kernel recomputes the acc spectra of every output window (acc times the plain scan's work).
 * Outputs are [rows][out_stride] with column w; any of the three may be NULL.
 *
 * lora_detect_scan_acc_windows: host arithmetic only; Wa.
 * lora_detect_scan_acc_batch: one kernel on `stream`, nothing allocated or synchronised, columns
 * 0 .. Wa-1 of every output given fully written and nothing beyond.  rows == 0, Wa == 0 or no
 * output: no launch.  LORA_EINVAL before any HIP call: lora_detect_scan_batch's cases, acc
 * outside 1..8, acc > 1 with hop not dividing step, out_stride < Wa with an output given.
 * Returns Wa. */
int64_t lora_detect_scan_acc_windows(const lora_demod_plan* plan, int64_t row_len, int64_t hop, int64_t acc);
int64_t lora_detect_scan_acc_batch(lora_demod_plan* plan, const float* iq, int64_t rows, int64_t row_len,
                                   int64_t row_stride, int64_t hop, int64_t acc, int conj, float* power,
                                   float* power_avg, uint16_t* index, int64_t out_stride, void* stream);

/* The preamble finder: frame starts and integer carrier offsets from two accumulating scans of
 * the same rows with the same hop by a dechirping plan at bw 125 kHz: up_* with acc = m =
 * params.acc_up and conj = 0 (Wu windows), dn_* with acc = 2 and conj = 1 (Wd windows).  A
 * window d chips late under an offset of c bins sees bin d + c on the up side and d - c on the
 * down side, which is what separates the two.  With N = 2^sf, step = N*osr, k = step / hop >= 4,
 * tail = 9*step/4: for down window w with (2+m)*k <= w, w + k < Wd and u = w - (2+m)*k < Wu, all
 * of these must hold:
 *   1. dn_power[w] - dn_avg[w] >= thresh_dn_db and up_power[u] - up_avg[u] >= thresh_up_db (one
 *      fp32 subtraction each; NaN fails, +inf passes);
 *   2. dn_power[w] >= dn_power[w-k] and dn_power[w] > dn_power[w+k]: the symbol where both summed
 *      windows lie on down-chirps;
 *   3. s = (up_index[u] + dn_index[w]) mod N, minus N when s >= N/2; d = floor(s / 2);
 *      c = (up_index[u] - d) mod N, minus N when c >= N/2; |c| <= max_cfo_bins - which rejects the
 *      (d +- N/2, c +- N/2) alias that windows near a quarter symbol off produce;
 *   4. start = w*hop - d*osr - 2*step, the first sync symbol, with start >= 0 and
 *      start + 10*step + tail <= row_len.
 * A candidate is listed in increasing w, unless its (start, c) pair equals that of the previous
 * window that passed 1-4, listed or not.  Per row: count (may exceed capacity), starts and
 * cfo_bins [rows][capacity], -1 and 0 in the empty slots.
 * One kernel on `stream` of params.device, one workgroup per row, nothing allocated or
 * synchronised, every output fully written; rows == 0: no launch.  LORA_EINVAL before any HIP
 * call: a NULL params or count, NULL starts or cfo_bins with capacity > 0, NULL metrics with
 * windows to test, sf outside 7..12, osr outside 1..65536, hop not dividing step or k < 4,
 * acc_up outside 2..8, max_cfo_bins outside 0 .. N/4 - 1, negative sizes, a stride below its
 * window count with more than one row, Wu or Wd >= 2^31, rows >= 2^31.  Returns rows. */
typedef struct {
  unsigned sf;
  unsigned osr;
  int64_t hop;
  int acc_up;
  float thresh_up_db;
  float thresh_dn_db;
  int max_cfo_bins;
  int device;
} lora_preamble_params;
int64_t lora_find_preamble_batch(const lora_preamble_params* params, const float* up_power, const float* up_avg,
                                 const uint16_t* up_index, int64_t Wu, int64_t up_stride, const float* dn_power,
                                 const float* dn_avg, const uint16_t* dn_index, int64_t Wd, int64_t dn_stride,
                                 int64_t rows, int64_t row_len, int64_t capacity, int64_t* starts,
                                 int32_t* cfo_bins, int32_t* count, void* stream);

/* lora_select_frames_batch's pass for preambled frames, by the same kernel: a frame ends at
 * start + (2 + nsym)*step + tail (the slot is accepted when that is <= row_len, and first becomes
 * it), and one int32 per slot, cand_word [rows][slots], is carried to the accepted slot's
 * out_word [rows][capacity] (0 in the empty slots); cand_word and out_word may both be NULL.
 * tail == 0 without words is lora_select_frames_batch.  LORA_EINVAL as that entry's, and for
 * tail < 0 or only one of cand_word (with slots > 0) and out_word (with capacity > 0) given. */
int64_t lora_select_preamble_batch(const int64_t* cand_starts, const int32_t* cand_word, const int32_t* status,
                                   const int32_t* nsym, int64_t rows, int64_t slots, const int64_t* first,
                                   int64_t row_len, int64_t step, int64_t tail, int64_t max_symbols,
                                   int64_t capacity, int64_t* starts, int32_t* out_word, int32_t* out_nsym,
                                   int32_t* count, int64_t* end, int device, void* stream);

/* Digital down-converter bank: one wideband stream in, `channels` streams at the demodulator's
 * rate out, from one read of the wideband data.  The reference has no channelizer; this
 * definition is the library's own (like the finder's rule and the soft bits).
 *   iq    `rows` rows of `row_len` complex samples, row r at iq + 2*r*row_stride floats (device);
 *   taps  `ntaps` real fp32 values h[j] (device);
 *   nco   `period` complex fp32 values w[m] = (wr[m], wi[m]) (device): the oscillator table is
 *         an input, normally exp(-2 pi i m / period) rounded to fp32, so bit parity depends on
 *         nobody's cosine;
 *   steps a HOST array of `channels` ints k_c: channel c is centred k_c / period cycles per
 *         input sample above the tuner.  Any int; each is reduced mod `period` (to 0 .. period-1)
 *         on the host and travels in the kernel's arguments, so the call can be captured in a
 *         graph;
 *   out   [rows][channels][out_stride] complex samples: output t of channel c of row r is at
 *         out + 2*((r*channels + c)*out_stride + t) floats (device).
 * A row gives W = row_len < ntaps ? 0 : (row_len - ntaps) / decim + 1 outputs per channel and
 * no output reads past its row.  All arithmetic is fp32, one rounding per operation, no
 * contraction.  For sample n of a row, m = (k_c * (first_sample + n)) mod period (in integers,
 * non-negative):
 *   zr = xr*wr[m] - xi*wi[m]        zi = xr*wi[m] + xi*wr[m]
 * and for output t both accumulators start at +0.0f and, for j = 0 .. ntaps-1 in this order,
 *   yr = yr + h[j]*zr[t*decim + j]    yi = yi + h[j]*zi[t*decim + j].
 * Infinities and NaN propagate as this arithmetic makes them; there is no special case.  (Where
 * a result is NaN, its sign and payload are the processor's choice, as IEEE 754 leaves them:
 * the GPU's subtraction, for one, returns a NaN subtrahend with its sign flipped.)
 * first_sample (>= 0) keeps the oscillator's phase continuous when a long recording is
 * processed in chunks: a chunk that starts at a multiple of decim and overlaps its predecessor
 * by ntaps - decim samples continues the predecessor's outputs.
 *
 * lora_channelize_outputs: host arithmetic only; W, or LORA_EINVAL for a negative row_len,
 * ntaps < 1 or decim < 1.
 * lora_channelize_batch: enqueues one kernel on `stream` of `device`, allocates and synchronises
 * nothing, needs no workspace, and fully writes columns 0 .. W-1 of every (row, channel) and
 * nothing beyond them.  rows == 0 or W == 0: no launch.  LORA_EINVAL, before any HIP call: a
 * NULL taps, nco, steps or out, a NULL iq with work to do, negative sizes or first_sample,
 * ntaps outside 1..512, decim outside 1..64, period outside 1..4096, channels outside 1..32,
 * row_len >= 2^31, row_stride < row_len with more than one row, out_stride < W, a grid beyond
 * 2^31 (rows * ceil(W / outputs per workgroup)).  Returns W. */
int64_t lora_channelize_outputs(int64_t row_len, int64_t ntaps, int64_t decim);
int64_t lora_channelize_batch(const float* iq, int64_t rows, int64_t row_len, int64_t row_stride,
                              int64_t first_sample, const float* taps, int64_t ntaps, int64_t decim,
                              const float* nco, int64_t period, const int32_t* steps, int64_t channels,
                              float* out, int64_t out_stride, int device, void* stream);

/* Rational-rate down-converter bank: lora_channelize_batch with an interpolation factor, for a
 * wideband rate that is decim / interp times the channel rate (2.4 MS/s to 125 kS/s is 5/96).
 * The reference has no channelizer; this definition is the library's own.  The arguments are
 * lora_channelize_batch's, plus `interp` (L); `decim` is M, and `taps` are `ntaps` real fp32
 * values h[j] of a prototype filter at L times the input rate.
 * Mixing is unchanged: for sample n of a row, m = (k_c * (first_sample + n)) mod period and
 *   zr = xr*wr[m] - xi*wi[m]        zi = xr*wi[m] + xi*wr[m].
 * Output t of a channel is the zero-stuffed correlation sum_j h[j] * zup[t*M + j], where
 * zup[v] = z[v / L] when L divides v; the zero terms are left out, not added:
 *   j0 = (-(t*M)) mod L, in 0 .. L-1;      n0 = (t*M + j0) / L;
 *   K  = j0 >= ntaps ? 0 : ceil((ntaps - j0) / L);
 * both accumulators start at +0.0f and, for i = 0 .. K-1 in this order,
 *   yr = yr + h[j0 + i*L]*zr[n0 + i]    yi = yi + h[j0 + i*L]*zi[n0 + i].
 * All arithmetic is fp32, one rounding per operation, no contraction.  A residue with K == 0
 * gives (+0.0f, +0.0f).  Infinities and NaN propagate as this arithmetic makes them, with
 * lora_channelize_batch's caveat about a NaN's sign and payload.
 * A row gives, with span = (row_len - 1)*L + 1,
 *   W = (row_len < 1 || span < ntaps) ? 0 : (span - ntaps) / M + 1
 * outputs per channel, and no output reads past its row.  At interp == 1 every formula here is
 * lora_channelize_batch's.
 * Chunks: a chunk continues its predecessor's outputs when it starts at input sample n0 with
 * n0 * L a multiple of M, is given first_sample = n0, and the predecessor is long enough to
 * hold all outputs before n0*L/M.
 *
 * lora_resample_outputs: host arithmetic only; W, or LORA_EINVAL for a negative row_len,
 * ntaps < 1, interp < 1, decim < 1 or a row_len * interp beyond 64 bits.
 * lora_resample_channelize_batch: enqueues one kernel on `stream` of `device`, allocates and
 * synchronises nothing, needs no workspace, and fully writes columns 0 .. W-1 of every (row,
 * channel) and nothing beyond them.  rows == 0 or W == 0: no launch.  LORA_EINVAL, before any
 * HIP call: lora_channelize_batch's argument rules with these limits - interp outside 1..16,
 * decim outside 1..256, interp > decim (a rate-reducing bank only), ntaps outside 1..4096,
 * ceil(ntaps / interp) > 512, period outside 1..4096, channels outside 1..32, row_len >= 2^31.
 * (2.048 MS/s to 125 kS/s is 125/2048: beyond these limits.)  Returns W. */
int64_t lora_resample_outputs(int64_t row_len, int64_t ntaps, int64_t interp, int64_t decim);
int64_t lora_resample_channelize_batch(const float* iq, int64_t rows, int64_t row_len, int64_t row_stride,
                                       int64_t first_sample, const float* taps, int64_t ntaps, int64_t interp,
                                       int64_t decim, const float* nco, int64_t period, const int32_t* steps,
                                       int64_t channels, float* out, int64_t out_stride, int device,
                                       void* stream);

/* Raw SDR samples: both banks reading the capture as the radio wrote it, so that the integer
 * bytes are the only read of it (no convert pass, no workspace, no second kernel).  `format`
 * is one of */
#define LORA_IQ_CS16 1 /* little-endian int16 I, Q: 4 bytes per sample (USRP, Pluto, LimeSDR, .sigmf-data) */
#define LORA_IQ_CS8 2  /* int8 I, Q: 2 bytes per sample (HackRF) */
#define LORA_IQ_CU8 3  /* uint8 I, Q: 2 bytes per sample (RTL-SDR) */
/* The reference has no channelizer; this definition, like the banks', is the library's own.
 * For a stored component v, the fp32 sample component is
 *   x = ((float)v - bias) * scale
 * all of it fp32, one rounding per operation, no contraction: the conversion of the integer is
 * exact, bias is 127.5f for cu8 (the subtraction is exact too) and +0.0f for the signed formats,
 * where the subtraction changes no bit and is left out, and the product is the one rounding.
 * `scale` is the caller's fp32 value and is not checked: infinities and NaN propagate as the
 * arithmetic makes them (scale = inf turns a zero component into NaN).  The usual scales are
 * 1/32768, 1/128 and 1/127.5.  xr and xi then enter the float entry's mixing and FIR formulas
 * unchanged, so the outputs equal, bit for bit, the float entry's on the converted samples.
 *
 * lora_channelize_raw_batch is lora_channelize_batch and lora_resample_channelize_raw_batch is
 * lora_resample_channelize_batch, argument for argument, limit for limit and rule for rule, with
 * `const void* iq, int format, float scale` in place of `const float* iq`:
 *   iq    `rows` rows of `row_len` samples of `format`; row r begins r*row_stride SAMPLES after
 *         iq (device).  row_stride, row_len and first_sample stay in complex samples.  iq need
 *         only be aligned to one sample - 4 bytes for cs16, 2 bytes for cs8 and cu8 - so any
 *         sample of a capture can be a row's first; the kernel loads two samples at a time on
 *         the grid of that size (8 bytes for cs16, 4 for cs8 and cu8) and loads singly the one
 *         sample that may hang over either end.
 * W (lora_channelize_outputs, lora_resample_outputs: they serve both), the output layout, the
 * chunking rule, graph capturability and the contract - one kernel on `stream` of `device`,
 * nothing allocated or synchronised, no workspace, columns 0 .. W-1 fully written and nothing
 * beyond them, rows == 0 or W == 0 no launch (and a NULL iq allowed) - are the float entries'.
 * LORA_EINVAL, before any HIP call: a `format` that is none of the three (0 included), an iq
 * that is not aligned to one sample, and every argument rule of the float counterpart.
 * Returns W.  Nothing here corrects what an SDR front end does to the samples (DC offset, IQ
 * imbalance): the conversion above is the whole of it. */
int64_t lora_channelize_raw_batch(const void* iq, int format, float scale, int64_t rows, int64_t row_len,
                                  int64_t row_stride, int64_t first_sample, const float* taps, int64_t ntaps,
                                  int64_t decim, const float* nco, int64_t period, const int32_t* steps,
                                  int64_t channels, float* out, int64_t out_stride, int device, void* stream);
int64_t lora_resample_channelize_raw_batch(const void* iq, int format, float scale, int64_t rows, int64_t row_len,
                                           int64_t row_stride, int64_t first_sample, const float* taps,
                                           int64_t ntaps, int64_t interp, int64_t decim, const float* nco,
                                           int64_t period, const int32_t* steps, int64_t channels, float* out,
                                           int64_t out_stride, int device, void* stream);

/* Synthesis bank: the inverse of the down-converter banks.  `channels` streams at the modulator's
 * rate in, one wideband stream out, from one kernel that writes each wideband sample once.  The
 * reference has no synthesiser; this definition, like the banks', is the library's own.
 *   in     `rows` x `channels` streams of `chan_len` complex samples: stream (r, c) is at
 *          in + 2*(r*channels + c)*in_stride floats (device);
 *   taps   `ntaps` real fp32 values h[j] of a prototype low-pass filter at the OUTPUT rate
 *          (device); a gain of `interp` makes up for the zero-stuffing;
 *   interp the integer up-sampling factor U;
 *   nco    `period` complex fp32 values w[m] = (wr[m], wi[m]) (device): an input, as for the
 *          banks; to put channel c at k_c / period cycles per output sample above the centre it
 *          is exp(+2 pi i m / period) rounded to fp32, the conjugate of the banks' table;
 *   steps  a HOST array of `channels` ints k_c, any int, each reduced mod `period` (to
 *          0 .. period-1) on the host; they travel in the kernel's arguments;
 *   gains  a HOST array of `channels` fp32 values g_c, which also travel in the kernel's
 *          arguments, so the call can be captured in a graph;
 *   first_sample (>= 0) the index of output 0 in the transmitted recording: it keeps the
 *          oscillators' phase continuous across chunks;
 *   out    `rows` rows: output t of row r is sample r*out_stride + t of out (device).
 * All arithmetic is fp32, one rounding per operation, no contraction, and every accumulator
 * starts at +0.0f.  With P = ceil(ntaps / U):
 *   1. the gain, once per input sample:   ar = g_c*xr        ai = g_c*xi
 *   2. polyphase interpolation, "valid" outputs only.  For output t: p = t mod U, q = t / U,
 *      K = p >= ntaps ? 0 : ceil((ntaps - p) / U), and for i = 0 .. K-1 in this order
 *        sr = sr + h[p + i*U]*ar[q + P-1 - i]    si = si + h[p + i*U]*ai[q + P-1 - i]
 *      (the zero-stuffed terms are never formed; K == 0 gives (+0.0f, +0.0f));
 *   3. the mix, m = (k_c * (first_sample + t)) mod period (in integers, non-negative):
 *        zr = sr*wr[m] - si*wi[m]        zi = sr*wi[m] + si*wr[m]
 *   4. the sum over the channels, c = 0 .. channels-1 in this order from +0.0f:
 *        yr = yr + zr        yi = yi + zi.
 * Infinities and NaN propagate as this arithmetic makes them, with lora_channelize_batch's
 * caveat about a NaN's sign and payload.
 * A row gives W = chan_len < P ? 0 : (chan_len - P + 1)*U outputs and no output reads outside
 * its streams.  Chunks: a chunk continues its predecessor's outputs when it overlaps it by P-1
 * channel samples and is given first_sample advanced by the predecessor's W.  Delay: channel
 * sample m is centred on output m*U + (ntaps-1)/2 - (P-1)*U.
 * Only an integer up-sampling factor is covered; a rational up-rate (interp / decim) is not.
 *
 * lora_synthesize_raw_batch is lora_synthesize_batch with `void* out, int format, float
 * inv_scale` in place of `float* out`: the row is stored as cs16, cs8 or cu8 samples (LORA_IQ_*
 * above; out_stride stays in samples).  Per component, from the y of step 4:
 *   v = y*inv_scale (one product);   for cu8 only v = v + 127.5f (one sum);
 *   code = clamp(rintf(v), lo, hi), ties to even, [lo, hi] the format's code range;
 *   a NaN v stores the format's zero: 0 for the signed formats, 128 for cu8.
 * inv_scale is the caller's fp32 value and is not checked; the usual values are 32768, 128 and
 * 127.5, all exact.  The bits stored equal this rule applied to lora_synthesize_batch's output.
 * (They equal a division by scale = 1 / inv_scale followed by the same rounding only where the
 * division and the product round alike: power-of-two scales, the cs16 and cs8 defaults.)
 * out need only be aligned to one sample (8 bytes of complex64, 4 of cs16, 2 of cs8 and cu8), so
 * any sample of a larger transmit buffer can be a row's first; the kernel stores 16 bytes at a
 * time where the address allows and single samples at a row's ragged ends, and the bits are
 * the same at every alignment.
 *
 * lora_synthesize_outputs: host arithmetic only; W, or LORA_EINVAL for a negative chan_len,
 * ntaps < 1, interp < 1 or a chan_len * interp beyond 64 bits.
 * lora_synthesize_batch, lora_synthesize_raw_batch: enqueue one kernel on `stream` of `device`,
 * allocate and synchronise nothing, need no workspace, and fully write columns 0 .. W-1 of every
 * row and nothing beyond them.  rows == 0 or W == 0: no launch (and NULL pointers allowed).
 * LORA_EINVAL, before any HIP call: negative sizes or first_sample, interp outside 1..64, ntaps
 * outside 1..512, period outside 1..4096, channels outside 1..32, chan_len * interp >= 2^31,
 * in_stride < chan_len with more than one stream, out_stride < W with more than one row, an out
 * that is not aligned to one sample, a `format` that is none of the three (0 included), a grid
 * beyond 2^31 (rows * ceil(W / 1024)), and with work to do a NULL in, taps, nco, steps, gains
 * or out.  Returns W. */
int64_t lora_synthesize_outputs(int64_t chan_len, int64_t ntaps, int64_t interp);
int64_t lora_synthesize_batch(const float* in, int64_t rows, int64_t chan_len, int64_t in_stride,
                              int64_t first_sample, const float* taps, int64_t ntaps, int64_t interp,
                              const float* nco, int64_t period, const int32_t* steps, const float* gains,
                              int64_t channels, float* out, int64_t out_stride, int device, void* stream);
int64_t lora_synthesize_raw_batch(const float* in, int64_t rows, int64_t chan_len, int64_t in_stride,
                                  int64_t first_sample, const float* taps, int64_t ntaps, int64_t interp,
                                  const float* nco, int64_t period, const int32_t* steps, const float* gains,
                                  int64_t channels, void* out, int format, float inv_scale, int64_t out_stride,
                                  int device, void* stream);

/* Channel impairment: what stands between the synthesis bank and the down-converter banks.  Rows
 * of complex64 in, the same rows out with a gain, a carrier offset and counter-based white
 * Gaussian noise applied, from one kernel that reads each sample once and writes it once.  The
 * reference's channel is three lines of host code in its AWGN test; this definition, like the
 * banks', is the library's own.
 *   in     `rows` rows of `row_len` complex samples, row r at in + 2*r*in_stride floats (device);
 *          NULL: noise-only rows - gain and rotation are skipped and sigma is required;
 *   first_sample, first_row (>= 0) the index of sample 0 in the recording and of row 0 among the
 *          recording's rows;
 *   seed   the noise generator's 64-bit key;
 *   gain, fcw, phase, sigma  device arrays of `rows` entries, each of which may be NULL.  A NULL
 *          array means that its stage's arithmetic is not performed at all (not performed with a
 *          neutral value); fcw is the carrier offset as a 32-bit frequency control word, one step
 *          fs / 2^32, phase the 32-bit starting phase, one step 2 pi / 2^32;
 *   out    `rows` rows: output t of row r is sample r*out_stride + t of out (device).  out == in
 *          is allowed, with equal strides.
 * in and out need only be aligned to one sample.  For row r and output t let n = first_sample + t
 * and R = first_row + r, both as 64-bit unsigned.  All float arithmetic is fp32, one rounding
 * per operation, no contraction; K = 0x1.921fb6p-30f (fp32 pi times 2^-31); sincosf and logf are
 * glibc's to the bit (|angle| <= pi everywhere), sqrtf is correctly rounded.
 *   1. the gain (gain given):             xr = g*xr        xi = g*xi
 *   2. the rotation (fcw or phase given, a missing one of the two counting as 0):
 *        p = (uint32)phase[r] + (uint32)fcw[r] * (uint32)n          modulo 2^32
 *        th = (float)(int32)p * K         (s, c) = sincosf(th)
 *        yr = xr*c - xi*s                 yi = xr*s + xi*c
 *      so the phase is continuous across chunks by construction;
 *   3. the noise (sigma given): Philox4x32-10 with the standard multipliers 0xD2511F53,
 *      0xCD9E8D57 and Weyl constants 0x9E3779B9, 0xBB67AE85, key (seed & 0xffffffff, seed >> 32),
 *      counter (b lo, b hi, R lo, R hi) with b = n >> 1.  Sample n takes words (0, 1) of the
 *      block when n is even and words (2, 3) when it is odd, as (w0, w1):
 *        u = (float)(2*(w0 >> 9) + 1) * 0x1p-24f      exact, in (0, 1)
 *        rad = sqrtf(-2.0f * logf(u))
 *        ph = (float)(int32)w1 * K        (s, c) = sincosf(ph)
 *        a = sigma*rad        nr = a*c        ni = a*s
 *        yr = yr + nr         yi = yi + ni    (in == NULL: the output is (nr, ni) itself)
 *      Each component is N(0, sigma^2) truncated at 5.77 sigma.  For a signal of amplitude A an
 *      SNR of snr dB is sigma = A * 10^(-snr/20) / sqrt(2);
 *   4. the store: complex64, or with lora_impair_raw_batch - `void* out, int format, float
 *      inv_scale` in place of `float* out` - cs16, cs8 or cu8 codes by exactly
 *      lora_synthesize_raw_batch's rule (v = y*inv_scale, + 127.5f for cu8, clamp(rintf(v)), a
 *      NaN stores the format's zero); out_stride stays in samples.
 * Infinities and NaN in `in` propagate as this arithmetic makes them, with
 * lora_channelize_batch's caveat about a NaN's sign and payload.
 * A sample's value depends on (seed, R, n) and its row's parameters alone - not on chunking,
 * row count, alignment or which lane computed it: one call over a row equals, bit for bit, any
 * split of it into calls with first_sample advanced, and likewise for rows and first_row.
 * A fractional delay, multipath, frequency drift and a sample-clock offset are
 * lora_propagate_batch's, the stage in front of this one.  Not covered by either: DC offset, IQ
 * imbalance or any other front-end effect, and time-varying path gains.  An integer delay is the
 * caller's slice.
 *
 * Both entries enqueue one kernel on `stream` of `device`, allocate and synchronise nothing,
 * need no workspace and write samples 0 .. row_len-1 of every row and nothing else.  rows == 0
 * or row_len == 0: no launch.  LORA_EINVAL, before any HIP call, first rule first: negative
 * sizes, first_sample or first_row; row_len >= 2^31; with more than one row an in_stride (in
 * given) or out_stride smaller than row_len; out == in with unequal strides; an in or out that
 * is not aligned to one sample; a `format` that is none of the three (0 included); a grid beyond
 * 2^31 (rows * ceil(row_len / 1024)); and with work to do a NULL out, in == NULL with sigma ==
 * NULL, or nothing to do at all (all four arrays NULL).  Returns row_len. */
int64_t lora_impair_batch(const float* in, int64_t rows, int64_t row_len, int64_t in_stride, int64_t first_sample,
                          int64_t first_row, uint64_t seed, const float* gain, const int32_t* fcw,
                          const int32_t* phase, const float* sigma, float* out, int64_t out_stride, int device,
                          void* stream);
int64_t lora_impair_raw_batch(const float* in, int64_t rows, int64_t row_len, int64_t in_stride,
                              int64_t first_sample, int64_t first_row, uint64_t seed, const float* gain,
                              const int32_t* fcw, const int32_t* phase, const float* sigma, void* out, int format,
                              float inv_scale, int64_t out_stride, int device, void* stream);

/* Propagation: what stands between the synthesis bank and the impairment stage.  Rows of
 * complex64 in, rows of complex64 out: every output is the sum of `paths` paths, each the
 * recording read at a fractional position - a delay, slid by a sample-clock offset - through a
 * table of 256 fractional-delay filters and weighted by a complex gain; then a carrier offset
 * that may drift.  One kernel; this definition, like the impairment's, is the library's own.
 *   in     `rows` rows of `in_len` complex samples, row r at in + 2*r*in_stride floats (device).
 *          Element j of a row is sample in_first + j of the recording; every sample of the
 *          recording outside [in_first, in_first + in_len) reads as (+0, +0).  NULL is allowed
 *          with in_len == 0;
 *   out    `rows` rows of `row_len` samples: output t of row r is sample r*out_stride + t of out
 *          (device) and is sample n = first_sample + t of the received recording.  out must not
 *          overlap in: this is a filter, not a map;
 *   paths  P, 1..8;  delay [rows][P] int64 (device), the delay of each path in units of 2^-32
 *          sample, |delay| <= 2^47;  gain [rows][P][2] fp32 (device), (re, im) of each path;
 *   sfo    [rows] int64 (device) or NULL (0): the sample-clock offset in units of 2^-32 sample
 *          per sample, |sfo| <= 2^20 (about 244 ppm);
 *   table  [256][taps] fp32 (device), the fractional-delay interpolator: row ph delays by
 *          taps/2 - 1 + ph/256 samples.  taps = T is even, 2..32;
 *   fcw, rate  [rows] int64 (device) or NULL: the carrier offset in units of fs / 2^64 and its
 *          drift in units of fs / 2^64 per sample;  phase [rows] int32 (device) or NULL: the
 *          starting phase, one step 2 pi / 2^32.
 * first_sample >= 0, in_first >= 0, first_sample + row_len <= 2^40, in_first <= 2^41 (a clock
 * offset moves the last positions 2^28 samples past 2^40), row_len < 2^31.  in and out need only be aligned to one sample.
 * The position, for row r, path p and output n, all in int64 (the limits exclude overflow):
 *     m  = -(delay[r][p] + sfo[r] * n)
 *     q  = m >> 32  (arithmetic, i.e. floor)      fr = (uint32)m      ph = fr >> 24
 *     j0 = n + q - (T/2 - 1)
 * so the path reads the recording at x = n + q + fr / 2^32, truncated to a 256th of a sample.
 * The sum, all fp32, one rounding per operation, no contraction, in this order, re(j) and im(j)
 * being sample j of the recording:
 *     sr = si = +0
 *     for t = 0 .. T-1:   sr = sr + table[ph][t] * re(j0 + t)     si = si + table[ph][t] * im(j0 + t)
 *     cr = gr*sr - gi*si            ci = gr*si + gi*sr
 * and over the paths, from yr = yi = +0, for p = 0 .. P-1:   yr = yr + cr     yi = yi + ci.
 * The rotation is performed only if one of fcw, rate, phase is given, a missing one counting as 0:
 *     tri = n(n-1)/2 modulo 2^64: whichever of n, n-1 is even is halved, then the two are
 *           multiplied modulo 2^64 (n = 0: 0)
 *     W   = ((uint64)(uint32)phase[r] << 32) + (uint64)fcw[r] * n + (uint64)rate[r] * tri  mod 2^64
 *     th  = (float)(int32)(W >> 32) * K           (s, c) = sincosf(th)
 *     yr' = yr*c - yi*s             yi' = yr*s + yi*c
 * with lora_impair_batch's K and sincosf: with rate == NULL and fcw = (int64)fcw32 << 32 the
 * rotation is lora_impair_batch's bit for bit.
 * Infinities and NaN in `in` propagate as this arithmetic makes them (a zero coefficient times
 * an infinity is a NaN), with lora_channelize_batch's caveat about a NaN's sign and payload.
 * A sample's value depends on (n, its row's parameters, the recording) alone: one call equals,
 * bit for bit, any split of it into calls with first_sample advanced, and a call on any `in`
 * window that still covers the taps of every path.
 * delay and sfo live on the device, so their ranges cannot be checked here: they are the
 * caller's contract (lora_phy_amd.stream checks them on the host).  Beyond them the samples are
 * not this definition's, but nothing outside `in`'s window and `out`'s rows is touched.
 * Not covered: time-varying path gains, and DC offset, IQ imbalance or any other front-end
 * effect.  The quantiser is lora_impair_raw_batch, which follows this stage.
 *
 * Enqueues one kernel on `stream` of `device`, allocates and synchronises nothing, needs no
 * workspace and writes samples 0 .. row_len-1 of every row and nothing else.  rows == 0 or
 * row_len == 0: no launch.  LORA_EINVAL, before any HIP call, first rule first: negative rows,
 * in_len, in_stride, in_first, row_len, first_sample or out_stride; row_len >= 2^31;
 * first_sample + row_len > 2^40 or in_first > 2^41; with more than one row an in_stride smaller
 * than in_len or an out_stride smaller than row_len; an in or out that is not aligned to one
 * sample; in and out that overlap; paths outside 1..8; taps odd or outside 2..32; with work to
 * do a NULL delay, gain, table or out, or a NULL in with in_len > 0; a grid beyond 2^31 (rows *
 * ceil((row_len + 1) / 1024)).  Returns row_len. */
int64_t lora_propagate_batch(const float* in, int64_t rows, int64_t in_len, int64_t in_stride, int64_t in_first,
                             int64_t row_len, int64_t first_sample, int64_t paths, const int64_t* delay,
                             const float* gain, const int64_t* sfo, const float* table, int64_t taps,
                             const int64_t* fcw, const int64_t* rate, const int32_t* phase, float* out,
                             int64_t out_stride, int device, void* stream);

/* lora_modulate for `frames` independent frames: symbols [frames][sym_count] ->
 * iq [frames][(sym_count+2)*N*osr] (2 sync up-chirps then one chirp per symbol,
 * phase-continuous within a frame, LoRaMod.cpp:8-41).  Returns samples per frame. */
int64_t lora_mod_batch(unsigned sf, unsigned osr, unsigned bw_hz, float amplitude, uint8_t sync,
                       const uint16_t* symbols, int64_t frames, int64_t sym_count, float* iq,
                       int device, void* stream);

/* ---- Payload codec on the device: symbols <-> bytes for F frames per call ----------------
 * Each call enqueues one kernel on `stream` of `device`, allocates and synchronises nothing,
 * needs no workspace and fully writes every output it is given (no buffer has to be cleared
 * first).  All buffers are device memory; rows are `*_stride` elements apart.  Parameters are
 * checked before any HIP call: a NULL required buffer, sf outside 6..12, rdd outside 0..4,
 * nbytes > 255 or a stride smaller than its row give LORA_EINVAL; frames == 0 is a no-op that
 * returns the per-frame count.  Optional outputs (crc_ok and the counters) may be NULL. */

/* lora_phy::lora_decode (phy.hpp:213-215, LoRaDecoder.cpp:8-19) for `frames` frames of
 * `sym_count` symbols: Hamming 8/4 decode of each symbol's low byte (decodeHamming84sx,
 * LoRaCodes.hpp:250-281), consecutive pairs giving one byte, high nibble first; an odd
 * trailing symbol is ignored.  payload [frames][payload_stride] receives n = sym_count / 2
 * bytes per frame.  Per frame, optionally: crc_ok[f] = 1 when n >= 4 and
 * payload[n-2] | payload[n-1] << 8 equals sx1272DataChecksum (LoRaCodes.hpp:92-105) of
 * payload[2 .. n-2), else 0 - the check of lora_phy::decode (phy.hpp:118-120,
 * phy.cpp:241-256); err_count[f] / bad_count[f] = symbols whose decode raised `error` / `bad`.
 * Returns n. */
int64_t lora_decode_batch(const uint16_t* symbols, int64_t frames, int64_t sym_count, int64_t sym_stride,
                          uint8_t* payload, int64_t payload_stride, uint8_t* crc_ok, int32_t* err_count,
                          int32_t* bad_count, int device, void* stream);

/* lora_phy::lora_encode (phy.hpp:209-211, LoRaEncoder.cpp:8-19) for `frames` payloads of
 * `nbytes` bytes: each byte becomes two Hamming 8/4 codewords (encodeHamming84sx,
 * LoRaCodes.hpp:229-242) used as symbols, high nibble first.  With append_crc != 0 the
 * sx1272DataChecksum of payload[2 .. nbytes) follows as two more bytes, low byte first, so that
 * lora_decode_batch reports crc_ok on the round trip.  Returns the symbols per frame,
 * 2 * (nbytes + (append_crc ? 2 : 0)). */
int64_t lora_encode_batch(const uint8_t* payload, int64_t frames, int64_t nbytes, int64_t payload_stride,
                          int append_crc, uint16_t* symbols, int64_t sym_stride, int device, void* stream);

/* The receive side of the coding chain around the demodulator, at coding rate 4 / (4 + rdd)
 * and PPM = sf, the inverse of lora_encode_chain_batch: Gray -> binary (grayToBinary16,
 * LoRaCodes.hpp:212-222), diagonal deinterleave of whole blocks of 4 + rdd symbols into sf
 * codewords each (diagonalDeterleaveSx, LoRaCodes.hpp:396-412; trailing symbols that do not
 * fill a block are ignored), de-whitening (Sx1272ComputeWhiteningLfsr with bit offset 0,
 * LoRaCodes.hpp:176-189), nibble decode by rdd (Hamming 8/4, Hamming 7/4, parity 6/4, parity
 * 5/4, the bare nibble; LoRaCodes.hpp:250-365), nibbles packed high first into `nbytes` bytes.
 * err_count[f] (optional) = codewords among the first 2 * nbytes that flagged an error (Hamming
 * 8/4's `bad` counts as one).  LORA_ERANGE when 2 * nbytes exceeds the codewords sym_count
 * yields.  Returns nbytes. */
int64_t lora_decode_chain_batch(int sf, int rdd, const uint16_t* symbols, int64_t frames, int64_t sym_count,
                                int64_t sym_stride, int64_t nbytes, uint8_t* payload, int64_t payload_stride,
                                int32_t* err_count, int device, void* stream);

/* lora_decode_chain_batch on soft bits: maximum-likelihood decoding of every codeword over its
 * 16 candidates.  llr is [frames][sym_stride][sf] floats (lora_demod_soft_bits_batch's layout,
 * sym_stride in symbols; pass llr + 2*sf and sym_count = total - 2 to skip the sync columns of
 * a LEGACY / API result).  With nb = 4 + rdd, only whole blocks of nb symbols are used:
 *   deinterleave (diagonalDeterleaveSx's map, LoRaCodes.hpp:396-412, applied to LLRs):
 *     L[blk*sf + (c + bit) % sf][bit] = llr[blk*nb + bit][c], bit < nb, c < sf;
 *   de-whiten (Sx1272ComputeWhiteningLfsr with bit offset 0, LoRaCodes.hpp:176-189, masked by
 *     0xFF >> (4 - rdd)): where bit b of byte j of the sequence is set, L[j][b] is negated;
 *   decode codeword j: for each nibble x = 0..15 with codeword e (LoRaCodes.hpp:229-371 by
 *     rdd), m(x) starts at +0.0f and, for b = 0 .. nb-1 in this order,
 *     m = m + (bit b of e ? L[j][b] : -L[j][b]) in fp32, no contraction.  best starts at -inf
 *     and the nibble at 0; x is scanned upward from 0 and taken where m(x) > best (strict), so
 *     the lowest nibble wins ties and a NaN (or -inf) metric never wins.  At rdd = 0 this is
 *     the sign of each LLR;
 *   nibbles are packed high first into `nbytes` bytes.
 * corrected[f] (optional) = codewords among the first 2 * nbytes whose chosen codeword differs
 * from the hard word (bit b = L[j][b] > 0) in any of the nb positions.  One kernel, nothing
 * allocated or synchronised, no workspace, every output fully written.  Parameter checks and
 * LORA_ERANGE as in lora_decode_chain_batch.  Returns nbytes. */
int64_t lora_decode_chain_soft_batch(int sf, int rdd, const float* llr, int64_t frames,
                                     int64_t sym_count, int64_t sym_stride, int64_t nbytes,
                                     uint8_t* payload, int64_t payload_stride,
                                     int32_t* corrected, int device, void* stream);

/* The transmit side of the same chain (the order of runners/lora_phy_vector_generate.cpp:
 * 189-223): bytes -> nibbles, high first -> codewords by rdd (LoRaCodes.hpp:229-371), padded
 * with zero codewords to a multiple of sf -> whitening (LoRaCodes.hpp:176-189) -> diagonal
 * interleave (diagonalInterleaveSx, LoRaCodes.hpp:376-394) -> Gray (binaryToGray16,
 * LoRaCodes.hpp:201-207).  Returns the symbols per frame (lora_chain_symbols). */
int64_t lora_encode_chain_batch(int sf, int rdd, const uint8_t* payload, int64_t frames, int64_t nbytes,
                                int64_t payload_stride, uint16_t* symbols, int64_t sym_stride, int device,
                                void* stream);

/* Symbols per frame of the chain for `nbytes` payload bytes: ceil(2 * nbytes / sf) * (4 + rdd)
 * (the block count of diagonalInterleaveSx, LoRaCodes.hpp:376-394).  Host arithmetic only, no
 * HIP call. */
int64_t lora_chain_symbols(int sf, int rdd, int64_t nbytes);

/* ---- Self-describing frames: an explicit header in front of the coding chain ---------------
 * A frame that states its own payload length, coding rate and CRC flag, so that a receiver
 * needs no frame length from its caller.  The reference has the two primitives an explicit
 * header exists for (headerChecksum, LoRaCodes.hpp:43-67; sx1272DataChecksum, LoRaCodes.hpp:
 * 92-105) but no header: the layout is this library's own, in the familiar LoRa arrangement (a
 * first block at rate 4/8 on sf - 2 bits per symbol, 5 header nibbles, a payload CRC16).  No
 * on-air interoperability is claimed; as in the reference there is no preamble or SFD.
 *
 * For sf in 7..12, rdd in 0..4, n in 0..255 payload bytes P and crc in {0, 1}:
 *   data bytes  D = P, then with crc the two bytes c & 0xFF, c >> 8, c = sx1272DataChecksum of
 *               all n bytes of P; data nibbles high first, ND = 2 * (n + 2 * crc) of them
 *   header      h0 = n, h1 = rdd << 1 | crc, h2 = headerChecksum({h0, h1}) (5 bits); nibbles
 *               h0 >> 4, h0 & 15, h1 & 15, h2 >> 4, h2 & 15
 *   block 0     sf - 2 codewords: Hamming 8/4 (LoRaCodes.hpp:229-242) of the five header
 *               nibbles, then of the first sf - 7 data nibbles (a zero codeword where the data
 *               has run out); codewords 5 onward are whitened (Sx1272ComputeWhiteningLfsr on
 *               them with bit offset 0 and rdd 4, LoRaCodes.hpp:176-189), the header's are not;
 *               diagonalInterleaveSx at PPM sf - 2, rdd 4 (LoRaCodes.hpp:376-394) gives 8
 *               symbols; binaryToGray16; << 2
 *   the rest    the K = max(ND - (sf - 7), 0) data nibbles from index sf - 7 on, exactly as
 *               lora_encode_chain_batch treats a payload except that the whitening starts at bit
 *               offset sf - 7: codewords by rdd, zero codewords up to B * sf, B = ceil(K / sf),
 *               whitening, diagonalInterleaveSx at PPM sf, binaryToGray16
 *   symbols     nsym = 8 + B * (4 + rdd) per frame (the modulator adds its two sync symbols)
 * Decode of a frame of which `avail` symbols are there:
 *   avail < 8: status SHORT, every field 0.  Otherwise the header's symbols are rounded to the
 *   nearest multiple of four bins, r = ((s + 2) >> 2) & (2^(sf-2) - 1) (a +-1 bin error is
 *   absorbed), then grayToBinary16, diagonalDeterleaveSx at PPM sf - 2, rdd 4 (LoRaCodes.hpp:
 *   396-412), decodeHamming84sx (LoRaCodes.hpp:250-281) of codewords 0..4.  The header is bad
 *   (status HEADER, every field 0) when any of the five raised `bad`, when nibble 3 exceeds 1,
 *   when headerChecksum({h0, h1}) differs from the received one, or when h1 >> 1 > 4.
 *   Otherwise nbytes, rdd, has_crc and nsym are set, and errors counts the header's codewords
 *   that raised `error` or `bad`.  Header-only mode ends here with status OK.
 *   Full decode: nsym > avail (or nbytes > max_bytes) is status SHORT, the fields set, the
 *   payload zeros.  Otherwise the inverse of the above gives D; errors also counts those of
 *   the ND data codewords that flagged an error (Hamming 8/4's `bad` counts as one); status is
 *   CRC when crc is set and the two received bytes differ from sx1272DataChecksum(P) - the
 *   payload is written all the same - else OK.  Payload bytes beyond nbytes are written 0. */
#define LORA_FRAME_OK 0
#define LORA_FRAME_HEADER 1
#define LORA_FRAME_SHORT 2
#define LORA_FRAME_CRC 3

/* nsym of a frame (above; headerChecksum's fields, LoRaCodes.hpp:43-67).  Host arithmetic
 * only, no HIP call.  sf outside 7..12, rdd outside 0..4, nbytes outside 0..255 or crc outside
 * {0, 1} is LORA_EINVAL, here and below. */
int64_t lora_frame_symbols(int sf, int rdd, int64_t nbytes, int crc);

/* Encode `frames` frames (the layout above; LoRaCodes.hpp:43-67, 92-105, 176-189, 229-371,
 * 376-394).  payload [frames][payload_stride] holds up to max_bytes bytes per frame, of which
 * frame f has nbytes[f] (device int32, clamped to 0..max_bytes; NULL: max_bytes each); rdd and
 * crc are per call.  symbols [frames][sym_stride]: columns 0 .. S-1 are written, S =
 * lora_frame_symbols(sf, rdd, max_bytes, crc), with 0 beyond the frame's own nsym; nsym[f]
 * (optional) receives that count.  One kernel, nothing allocated or synchronised, parameters
 * checked before any HIP call as for the codec above.  Returns S. */
int64_t lora_encode_frame_batch(int sf, int rdd, int crc, const uint8_t* payload, int64_t frames, int64_t max_bytes,
                                int64_t payload_stride, const int32_t* nbytes, uint16_t* symbols,
                                int64_t sym_stride, int32_t* nsym, int device, void* stream);

/* Decode `frames` frames (the decode above; LoRaCodes.hpp:43-67, 92-105, 176-189, 212-222,
 * 250-365, 396-412) from symbols [frames][sym_stride], of which frame f has avail[f] (device
 * int32, clamped to 0..sym_count; NULL: sym_count each).  Per frame, each optional: status
 * (LORA_FRAME_*), nbytes, rdd, has_crc, nsym, errors (int32).  payload [frames][payload_stride]
 * receives max_bytes (0..255) bytes per frame; a NULL payload selects header-only mode.  One
 * kernel, nothing allocated or synchronised, every output fully written.  Returns max_bytes
 * (0 in header-only mode). */
int64_t lora_decode_frame_batch(int sf, const uint16_t* symbols, int64_t frames, int64_t sym_count,
                                int64_t sym_stride, const int32_t* avail, int32_t* status, int32_t* nbytes,
                                int32_t* rdd, int32_t* has_crc, int32_t* nsym, int32_t* errors, uint8_t* payload,
                                int64_t max_bytes, int64_t payload_stride, int device, void* stream);

/* lora_decode_frame_batch on soft bits.  llr is [frames][sym_stride][sf] floats, the DATA columns
 * of a frame (lora_demod_soft_bits_frame_batch's layout with red_first = 2, red_count = 8; pass
 * llr + 2*sf): column 0 is the first header symbol and columns 0 .. 7 hold the reduced form.
 * avail, status, nbytes, rdd, has_crc, nsym, payload, max_bytes and header-only mode (a NULL
 * payload) are lora_decode_frame_batch's.  For a frame of which `avail` columns are there:
 *   avail < 8: status SHORT, every field 0, hdr_flips 0.  Otherwise
 *   block 0     L0[(c + bit) % (sf-2)][bit] = llr[bit][c], bit < 8, c < sf - 2
 *               (diagonalDeterleaveSx at PPM sf - 2, LoRaCodes.hpp:396-412, on LLRs); for
 *               codewords j >= 5 the sign of L0[j][b] is flipped where bit b of byte j - 5 of
 *               Sx1272ComputeWhiteningLfsr (bit offset 0, rdd 4, LoRaCodes.hpp:176-189) is set;
 *               the header's five are not flipped
 *   a codeword  of nb LLRs L[0 .. nb-1] at rate 4/(4 + r), nb = 4 + r: maximum likelihood over
 *               its 16 codewords with lora_decode_chain_soft_batch's metric - m(x) starts at
 *               +0.0f and, for b = 0 .. nb-1 in this order, m = m + (bit b of e(x) ? L[b] :
 *               -L[b]) in fp32, no contraction; x is scanned upward from best = -inf with a
 *               strict '>', so the lowest nibble wins a tie and a NaN metric never wins.  Its
 *               hard word is bit b = L[b] > 0.  Any float is a valid LLR; no NaN is written
 *   header      codewords 0 .. 4 of block 0 at r = 4 (Hamming 8/4, LoRaCodes.hpp:229-242) give
 *               the five nibbles; hdr_flips = the bit positions in which the five chosen
 *               codewords differ from their hard words (0 .. 40).  The header is bad (status
 *               HEADER, every field 0, hdr_flips still written) when nibble 3 exceeds 1, when
 *               headerChecksum({h0, h1}) (LoRaCodes.hpp:43-67) differs from the received one,
 *               when h1 >> 1 > 4, or when hdr_flips > max_flips.  (The hard gate tolerates one
 *               flipped bit in each of five codewords: max_flips = 5 is its like.  Without a
 *               limit the ML decoder maps every noise word to a codeword and only the 5-bit
 *               checksum is left to refuse it.)  Otherwise nbytes, rdd, has_crc and nsym are
 *               set; header-only mode ends here with status OK
 *   full decode nsym > avail (or nbytes > max_bytes) is status SHORT, the fields set, the payload
 *               zeros.  Otherwise data nibbles 0 .. sf-8 are codewords 5 onward of block 0 (r =
 *               4), and the others come from columns 8 .. nsym-1 exactly as
 *               lora_decode_chain_soft_batch treats a chain at the header's rdd, except that the
 *               whitening starts at bit offset sf - 7.  Nibbles, the CRC comparison, CRC and OK
 *               are lora_decode_frame_batch's; payload bytes beyond nbytes are written 0
 *   corrected   codewords whose chosen codeword differs from the hard word: among the header's
 *               five, plus (after a full decode) among the first ND data codewords; 0 with a bad
 *               header
 * hdr_flips (optional) int32 per frame.  max_flips outside 0 .. 40 is LORA_EINVAL; the other
 * parameter checks are lora_decode_frame_batch's.  One kernel, nothing allocated or
 * synchronised, no workspace, every output fully written.  This definition is the library's
 * own: the reference has no soft path.  Returns max_bytes (0 in header-only mode). */
int64_t lora_decode_frame_soft_batch(int sf, const float* llr, int64_t frames, int64_t sym_count,
                                     int64_t sym_stride, const int32_t* avail, int32_t* status, int32_t* nbytes,
                                     int32_t* rdd, int32_t* has_crc, int32_t* nsym, int32_t* corrected,
                                     int32_t* hdr_flips, int max_flips, uint8_t* payload, int64_t max_bytes,
                                     int64_t payload_stride, int device, void* stream);

/* Cut `slots` frames out of a stream: out[s][t] = flat[at[s] + t] for t < len[s], 0 for
 * len[s] <= t < cut (complex64 as interleaved floats, as lora_demod_batch takes them,
 * LoRaDemod.cpp:49-61; flat holds `total` samples).  at and len are device int64 arrays; a slot
 * with at[s] < 0 or at[s] >= total is all zeros, len is clamped to 0..cut and to the stream's
 * end: nothing at or beyond at[s] + len[s], or beyond flat + total, is read.  The zeros make a
 * slot's demodulation a function of its frame alone.  flat is 8-byte aligned (a frame starts at
 * any sample); out [slots][out_stride] and its rows are 16-byte aligned (out_stride even),
 * out_stride >= cut, else LORA_EINVAL.  One kernel, nothing allocated or synchronised, columns
 * 0 .. cut-1 of every row fully written.  Returns cut. */
int64_t lora_gather_frames_batch(const float* flat, int64_t total, const int64_t* at, const int64_t* len,
                                 int64_t slots, int64_t cut, float* out, int64_t out_stride, int device,
                                 void* stream);

/* Measurement hooks (bench.py): while enabled, every kernel lora_demod_batch launches
 * on this plan is bracketed by a pair of HIP events on the stream it runs on, for up
 * to `max_calls` calls.  Stages: 0 = frame max, 1 = estimate + sync symbols (with the
 * speculative pipeline: its pre-pass and certification kernels), 2 = symbol demod.
 * lora_demod_profile_read waits for the recorded events and returns, per stage, the
 * summed kernel ms over the recorded calls (stage_ms[3]) and the number of calls
 * recorded.  No effect on results. */
int lora_demod_profile_enable(lora_demod_plan* plan, int max_calls);
int lora_demod_profile_read(lora_demod_plan* plan, float* stage_ms, int* calls);

/* Which kernels the plan's last lora_demod_batch call launched (bit mask, for tests and
 * measurement): the speculative single-read pipeline is SPEC + ESTIMATE + DEMOD; the
 * three-launch path is FRAME_MAX (LEGACY) + ESTIMATE + DEMOD; GENERIC marks the LDS
 * estimate kernel (frames with fewer than two whole symbols).  0 before the first call.
 * Host-side bookkeeping only.  (Bit 8 belonged to a frame-resident kernel that measured
 * slower and was removed; it is never set.) */
#define LORA_KERNEL_FRAME_MAX 1
#define LORA_KERNEL_ESTIMATE 2
#define LORA_KERNEL_DEMOD 4
#define LORA_KERNEL_GENERIC 16
#define LORA_KERNEL_FRAME_MAX_WAVE 32 /* with FRAME_MAX: the one-wave-per-frame variant (short frames) */
#define LORA_KERNEL_SPEC 64 /* the speculative single-read pipeline (with ESTIMATE + DEMOD) */
int lora_demod_last_kernels(const lora_demod_plan* plan);

/* LEGACY frames at osr 1-4 with either window (none or Hann), SF 6-12, of 3 .. 2 + 4 * 2^SF symbols (SF7: 514),
 * run as a speculative single-read pipeline (LORA_KERNEL_SPEC) - and LORA_MODE_API frames at osr 1 (the exact
 * estimate first, then every data symbol rotated with the hardware sine/cosine and certified or recomputed
 * exactly; phy.cpp:178-239) and LORA_MODE_RAW frames at osr 1, SF 6-9 (every symbol through the same symbol
 * pass with no rotation, certified against the transforms' rounding or recomputed): the offset estimate on
 * unscaled samples, every
 * data symbol demodulated once while the frame maximum is reduced from the same read, then
 * the exact estimate, with each data symbol either certified by a rounding bound on its
 * argmax margin or recomputed exactly - the outputs equal the reference's (LoRaDemod.cpp:
 * 49-195) either way.  This returns how many data symbols this plan has recomputed so far
 * (synchronises the device; for tests and diagnostics).  LORA_MI355X_SPEC=0 disables the
 * pipeline (three launches: frame max, estimate, demod). */
int64_t lora_demod_spec_recomputed(lora_demod_plan* plan);

/* What the pipeline's certification saw and decided in the lora_demod_batch call that just ran
 * on `workspace` (a read-only diagnostic for tests and tools; host code only, no kernel).
 * `plan`, `workspace`, `workspace_bytes`, `frames` and `frame_len` are that call's; the caller
 * answers for that, the entry can only check that the plan's last call took the pipeline
 * (LORA_KERNEL_SPEC in lora_demod_last_kernels) and that the workspace holds the layout.  It
 * synchronises `stream` (the call's), then copies into the caller's host buffers:
 *   fp_spec[f], fp[f]  the offsets the symbol pass used (the pre-pass estimate on unscaled
 *                      samples) and the exact ones (LoRaDemod.cpp:79-135 on the normalised
 *                      frame), f < frames.  LORA_MODE_API: the symbol pass runs with the exact
 *                      offsets, both are those; LORA_MODE_RAW: there are none, both are zero.
 *   max_slot[f]        float bits: the pre-pass's max(|I|,|Q|) over the samples outside the
 *                      data-symbol windows that fp_spec implies ([0, 2 step), a positive t_off's
 *                      [2 step, 2 step + t_off), the frame's tail).  API and RAW: 0 (not taken).
 *   entries[f * total + s][2]  symbol s < total = frame_len / step of frame f: the margin
 *                      |X1| - |X2| between the top bin and the runner-up (float bits), then for
 *                      a data symbol its window's max(|I|,|Q|) (float bits), for a LEGACY sync
 *                      symbol (s < 2) the speculative index.  API: entries 0 and 1 are zero
 *                      (the estimate kernel demodulated the sync symbols exactly).
 *   list[i][2]         the symbols the certification rejected and k_spec_fix recomputed, as
 *                      (frame, symbol of the frame), stripe after stripe; symbol 0xFFFFFFFF is
 *                      the frame's sync pair (LEGACY).
 * Every pipeline (LEGACY, API, RAW) zeroes the list's counters before its certification and
 * k_spec_fix only reads them, so the list stays readable until the workspace's next call.
 * Returns the number of listed entries - what that call added to lora_demod_spec_recomputed.
 * Before any use of the plan: LORA_EINVAL for a NULL plan / workspace / out ("null argument"),
 * for frames <= 0 or frame_len < 0, for a NULL buffer in `out`; LORA_ERANGE for frame_cap <
 * frames.  Then LORA_EINVAL when the plan's last call did not take the pipeline, LORA_ERANGE
 * for sym_cap < frames * total, for a workspace smaller than lora_demod_workspace_bytes, and -
 * after the counters were read - for list_cap below the list's length; LORA_EIO for a HIP
 * error or a counter beyond the list's capacity (not this call's workspace). */
typedef struct lora_spec_frame {
  float cfo, time_offset; /* the frame's outputs */
  float rate;             /* rotation per sample, -2 pi cfo / N */
  float scale;            /* 1 / max when scaled, else 1 */
  int32_t t_off;          /* round(time_offset) */
  int32_t scaled;         /* the frame's maximum exceeds 1 */
  int32_t reserved[2];
} lora_spec_frame;
typedef struct lora_spec_trace_out {
  lora_spec_frame* fp_spec; /* [frame_cap] */
  lora_spec_frame* fp;      /* [frame_cap] */
  uint32_t* max_slot;       /* [frame_cap] */
  uint32_t* entries;        /* [sym_cap][2] */
  uint32_t* list;           /* [list_cap][2] */
  int64_t frame_cap, sym_cap, list_cap;
} lora_spec_trace_out;
int64_t lora_demod_spec_trace(const lora_demod_plan* plan, const void* workspace, size_t workspace_bytes,
                              int64_t frames, int64_t frame_len, const lora_spec_trace_out* out, void* stream);

/* Choose the plan's path explicitly (instead of the process-wide LORA_MI355X_SPEC read at
 * plan creation): speculative = 1 runs the speculative single-read pipeline wherever it
 * covers the configuration (the default), 0 always the three-launch exact path.  Both give
 * the reference's outputs; the second is the pipeline's checker in the tests.  Returns 0. */
int lora_demod_plan_set_pipeline(lora_demod_plan* plan, int speculative);

/* Diagnostics of the C++ drop-in's private AQL queue (liblora_phy.so): with
 * LORA_MI355X_AQL_PROFILE=1 set before the queue is created, every dispatch is timestamped
 * and this returns the last call's timeline in microseconds relative to its doorbell:
 * out[0] = packets n, out[1 + 2i], out[2 + 2i] = packet i's start and end on the GPU,
 * out[1 + 2n] = when the host saw the completion.  Returns the doubles written (0 when
 * nothing was profiled or cap < 2n + 2). */
int lora_aql_last_profile(double* out, int cap);

/* Thread-local text of the last error ("" if none). */
const char* lora_last_error(void);

/* Library version string. */
const char* lora_version(void);

#ifdef __cplusplus
}
#endif
#endif /* LORA_MI355X_H */
