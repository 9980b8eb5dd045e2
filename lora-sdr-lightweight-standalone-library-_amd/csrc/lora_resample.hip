// lora_resample.hip — the rational-rate down-converter bank (lora_resample_channelize_batch).
//
// lora_channelize_batch with an interpolation factor: every sample is mixed with each
// channel's oscillator, the mixed stream is zero-stuffed to `interp` times its rate, filtered
// with `ntaps` real taps at that rate and decimated by `decim`.  The zero terms are never
// formed: output t is the sum over i < K of h[j0 + i*interp] * z[n0 + i] with the header's
// j0, n0 and K, in that order from +0.0f, fp32, one rounding per operation, no contraction
// (tests/resample_checker.py restates it in numpy and the GPU tests compare bits).  The
// reference has no channelizer; the definition is this library's own.
//
// Outputs with equal r = t mod interp share one sub-filter, and their first samples are
// exactly `decim` apart: t = r + interp*u starts at u*decim + off[r], off[r] = ceil(r*decim /
// interp) < decim.  Each residue is therefore the integer bank's problem, and the kernel keeps
// that bank's structure (csrc/lora_channelize.hip).  A workgroup owns `tile` consecutive u, all
// `interp` residues of them, of every channel of one row.  It reads the samples they cover once,
// with 16-byte loads, and mixes each sample once per channel into LDS by phase: sample s of the
// tile sits at [s % decim][s / decim], a row of pitch ps per phase, so that the read of one tap
// for consecutive u is a read of consecutive LDS entries.  In the FIR a wavefront takes one
// residue at a time, one u per lane and two channels per lane (64 / tile channel lanes, so a
// group of 2 * 64 / tile channels); the residue's taps h[j0 + i*interp] are loaded 64 at a time,
// one per lane, and handed round by readlane.  The interp * ceil(cg / group) (residue, channel
// group) items of a pass are dealt round the workgroup's wavefronts.  The per-residue constants
// (j0, off, K) come from the host in the kernel's arguments, as the steps do.
//
// Geometry (resample_geometry below; tests restate it).  reach = max over r of off[r] + K[r]:
// the samples a u reaches from u*decim on.  One channel takes
//   entries(tile) = decim * (tile + (reach - 1) / decim)
// LDS entries of 8 bytes.  tile is the largest of 64, 32, 16, 8 with channels * entries(tile)
// <= 8192 (64 KiB), and 8 if none is; cg = min(channels, 8192 / entries(tile)) channels are
// taken per pass, each pass re-reading the tile's samples.  entries(8) <= 8*256 + 255 + 512, so
// cg >= 2.  At interp == 1 this is the integer bank's rule.  The workgroup has 4 to 8 wavefronts:
// the fewest with which the items = interp * ceil(cg / (2 * 64 / tile)) of a full pass take the
// fewest rounds, ceil(items / wavefronts) (5 wavefronts for interp 5 with one channel group,
// where 4 would leave three of them idle while the first does a second residue).
//
// The kernel's body is a template over the sample format (csrc/lora_iq_format.h):
// k_channelize_resample is its complex64 instance, for lora_resample_channelize_batch, and
// k_channelize_raw_resample<format> its cs16, cs8 and cu8 instances, for
// lora_resample_channelize_raw_batch, whose integer samples become fp32 in the load in front of
// the mixing.  The mix stage, the oscillator's arithmetic, the search for tile and cg and the
// argument rules common to both down-converter banks are csrc/lora_bank.h's.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/lora_mi355x.h"
#include "lora_bank.h"

#pragma clang fp contract(off)

namespace lora {
namespace {

constexpr int kMinWaves = 4, kMaxWaves = 8, kMaxThreads = 64 * kMaxWaves;
constexpr int kMaxInterp = 16, kMaxDecim = 256, kMaxTaps = 4096, kMaxPhaseTaps = 512;

struct ResArgs {
  const void* iq;  // samples of the kernel's format
  const float* taps;
  const cf* nco;
  cf* out;
  int64_t row_stride, out_stride, W, gpr;
  int ntaps, interp, decim, period, channels;
  int first_mod;  // first_sample mod period
  int tile, lg_tile, ps, cg, threads;
  float inv_decim, inv_period;
  int steps[kMaxChannels];  // each in 0 .. period-1
  // residue r = t mod interp: first tap, first sample past u*decim, taps
  int j0[kMaxInterp], off[kMaxInterp], K[kMaxInterp];
  float scale;  // of an integer format's samples
};

template <int F>
__device__ __forceinline__ void resample_tile(const ResArgs& a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  v2f* Z = reinterpret_cast<v2f*>(smem);  // [cg][decim][ps]
  const int tid = threadIdx.x;
  const int64_t row = (int64_t)blockIdx.x / a.gpr;
  const int64_t u0 = ((int64_t)blockIdx.x - row * a.gpr) * a.tile;
  const int64_t t0 = u0 * a.interp;  // the tile's first output, < W
  const int64_t tend = a.W - t0 < (int64_t)a.tile * a.interp ? a.W : t0 + (int64_t)a.tile * a.interp;
  // the tile's first sample and how many it covers.  Output t reads no sample past
  // (t*decim + ntaps - 1) / interp, which grows with t and for t = W - 1 is inside the row
  // ((W-1)*decim + ntaps <= (row_len-1)*interp + 1); and no further than reach - 1 past its
  // u*decim, so cnt <= (tile-1)*decim + reach: every s below has its entry in Z.
  const int64_t n0 = u0 * a.decim;  // < row_len < 2^31
  const int cnt = (int)(((tend - 1) * a.decim + a.ntaps - 1) / a.interp - n0) + 1;
  const int chs = a.decim * a.ps;
  // the oscillator's position at the tile's first sample: (first_sample + n0) mod period
  const unsigned p0 = ((unsigned)a.first_mod + (unsigned)(n0 % a.period)) % (unsigned)a.period;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ul = lane & (a.tile - 1), cl = lane >> a.lg_tile, ncl = 64 >> a.lg_tile;
  const float* __restrict__ taps = a.taps;
  const cf* __restrict__ nco = a.nco;

  for (int c0 = 0; c0 < a.channels; c0 += a.cg) {
    const int nc = a.channels - c0 < a.cg ? a.channels - c0 : a.cg;
    if (c0) __syncthreads();  // the previous pass's FIR has read Z

    // every sample of the tile, mixed for the pass's channels.  Pairs of samples on the grid of a
    // pair's size (16 bytes of complex64); a pair that hangs over either end is loaded singly
    const MixStage<ResArgs> mix{a, nco, Z, p0, c0, nc, chs};
    load_samples<F>(a.iq, row * a.row_stride + n0, cnt, a.scale, tid, a.threads, mix);
    __syncthreads();

    // output t0 + ul*interp + r of channels c and c + ncl: tap i of residue r meets sample
    // ul*decim + off + i, entry [(off + i) % decim][ul + (off + i) / decim].  Every lane of the
    // wavefront runs the loop, because every lane's tap is read by readlane; a lane with no
    // output (t >= W, or no channel left) works on entries inside Z that belong to others or
    // were never written, and stores nothing.
    const int items = a.interp * ((nc + 2 * ncl - 1) / (2 * ncl)), waves = a.threads >> 6;
    for (int item = wave; item < items; item += waves) {
      const int r = item % a.interp, cb = item / a.interp * 2 * ncl;
      const int j0 = a.j0[r], off = a.off[r], K = a.K[r];
      const int64_t t = t0 + (int64_t)ul * a.interp + r;
      const bool live = t < a.W;
      const int c = cb + cl;
      const bool pair = cb + ncl < nc;  // the wavefront has a second channel to do
      const bool one = live && c < nc, two = live && c + ncl < nc;
      const v2f* z0 = Z + (c < nc ? c : 0) * chs + ul;
      const v2f* z1 = Z + (c + ncl < nc ? c + ncl : 0) * chs + ul;
      v2f y0 = {0.0f, 0.0f}, y1 = {0.0f, 0.0f};
      // 64 taps at a time, one per lane, handed round by readlane; `at` walks the phase rows
      int ph = off, at = off * a.ps;  // off < decim
      for (int ib = 0; ib < K; ib += 64) {
        const int n = K - ib < 64 ? K - ib : 64;
        const int hv = lane < n ? __float_as_int(taps[j0 + (ib + lane) * a.interp]) : 0;
        auto step = [&]() {
          at += a.ps;
          if (++ph == a.decim) {
            ph = 0;
            at -= a.decim * a.ps - 1;
          }
        };
        if (pair) {
          for (int jj = 0; jj < n; ++jj) {
            const float h = __int_as_float(__builtin_amdgcn_readlane(hv, jj));
            y0 = y0 + h * z0[at];
            y1 = y1 + h * z1[at];
            step();
          }
        } else {
          for (int jj = 0; jj < n; ++jj) {
            const float h = __int_as_float(__builtin_amdgcn_readlane(hv, jj));
            y0 = y0 + h * z0[at];
            step();
          }
        }
      }
      v2f* o = reinterpret_cast<v2f*>(a.out) + ((row * a.channels + c0 + c) * a.out_stride + t);
      if (one) *o = y0;
      if (two) o[(int64_t)ncl * a.out_stride] = y1;
    }
  }
}

__global__ void __launch_bounds__(kMaxThreads) k_channelize_resample(ResArgs a) { resample_tile<kIqCf32>(a); }

template <int F>
__global__ void __launch_bounds__(kMaxThreads) k_channelize_raw_resample(ResArgs a) {
  resample_tile<F>(a);
}

int64_t resample_outputs(int64_t row_len, int64_t ntaps, int64_t interp, int64_t decim) {
  if (row_len < 1) return 0;
  const int64_t span = (row_len - 1) * interp + 1;
  return span < ntaps ? 0 : (span - ntaps) / decim + 1;
}

// The per-residue constants of the header's definition, and reach = max(off + K)
int residues(int ntaps, int interp, int decim, int* j0, int* off, int* K) {
  int reach = 0;
  for (int r = 0; r < interp; ++r) {
    j0[r] = (interp - (r * decim) % interp) % interp;
    off[r] = (r * decim + j0[r]) / interp;
    K[r] = j0[r] >= ntaps ? 0 : (ntaps - j0[r] + interp - 1) / interp;
    if (off[r] + K[r] > reach) reach = off[r] + K[r];
  }
  return reach;
}

// u per workgroup, channels per pass and wavefronts per workgroup (the file header's rule)
void resample_geometry(int reach, int interp, int decim, int channels, int& tile, int& cg, int& waves) {
  channel_geometry(reach, decim, channels, tile, cg);
  const int group = 2 * (64 / tile), items = interp * ((cg + group - 1) / group);
  waves = kMinWaves;
  for (int w = kMinWaves + 1; w <= kMaxWaves; ++w)
    if ((items + w - 1) / w < (items + waves - 1) / waves) waves = w;
}

// Both entries: `format` is kIqCf32 for lora_resample_channelize_batch, else a checked LORA_IQ_*
int64_t resample_channelize(const void* iq, int format, float scale, int64_t rows, int64_t row_len,
                            int64_t row_stride, int64_t first_sample, const float* taps, int64_t ntaps,
                            int64_t interp, int64_t decim, const float* nco, int64_t period, const int32_t* steps,
                            int64_t channels, float* out, int64_t out_stride, int device, void* stream) {
  if (const char* bad = down_args_error(taps, nco, steps, out, rows, row_len, row_stride, out_stride, first_sample))
    return set_last_error(LORA_EINVAL, bad);
  if (interp < 1 || interp > kMaxInterp) return set_last_error(LORA_EINVAL, "interp must be in 1..16");
  if (decim < 1 || decim > kMaxDecim) return set_last_error(LORA_EINVAL, "decim must be in 1..256");
  if (interp > decim) return set_last_error(LORA_EINVAL, "interp must not exceed decim: a rate-reducing bank only");
  if (ntaps < 1 || ntaps > kMaxTaps) return set_last_error(LORA_EINVAL, "ntaps must be in 1..4096");
  if ((ntaps + interp - 1) / interp > kMaxPhaseTaps)
    return set_last_error(LORA_EINVAL, "ceil(ntaps / interp) must be <= 512");
  if (const char* bad = down_shape_error(period, channels, rows, row_len, row_stride))
    return set_last_error(LORA_EINVAL, bad);
  const int64_t W = resample_outputs(row_len, ntaps, interp, decim);  // (row_len - 1) * interp < 2^35
  ResArgs a{};
  const int reach = residues((int)ntaps, (int)interp, (int)decim, a.j0, a.off, a.K);
  int waves = 0;
  resample_geometry(reach, (int)interp, (int)decim, (int)channels, a.tile, a.cg, waves);
  a.threads = 64 * waves;
  a.W = W;
  a.gpr = ((W + interp - 1) / interp + a.tile - 1) / a.tile;
  if (const char* bad = down_output_error(out_stride, W, rows, a.gpr)) return set_last_error(LORA_EINVAL, bad);
  if (rows == 0 || W == 0) return W;
  if (!iq) return set_last_error(LORA_EINVAL, "null iq");
  a.iq = iq;
  a.scale = scale;
  a.taps = taps;
  a.nco = reinterpret_cast<const cf*>(nco);
  a.out = reinterpret_cast<cf*>(out);
  a.row_stride = row_stride;
  a.out_stride = out_stride;
  a.ntaps = (int)ntaps;
  a.interp = (int)interp;
  a.decim = (int)decim;
  a.period = (int)period;
  a.channels = (int)channels;
  a.first_mod = (int)(first_sample % period);
  for (a.lg_tile = 0; (1 << a.lg_tile) < a.tile; ++a.lg_tile) {
  }
  a.ps = a.tile + (reach - 1) / a.decim;
  a.inv_decim = 1.0f / (float)a.decim;
  a.inv_period = 1.0f / (float)a.period;
  bank_steps(steps, a.channels, period, a.steps);
  const size_t lds = (size_t)a.cg * channel_entries(a.tile, reach, a.decim) * sizeof(cf);
  void (*const kernel)(ResArgs) = format == LORA_IQ_CS16  ? k_channelize_raw_resample<LORA_IQ_CS16>
                                  : format == LORA_IQ_CS8 ? k_channelize_raw_resample<LORA_IQ_CS8>
                                  : format == LORA_IQ_CU8 ? k_channelize_raw_resample<LORA_IQ_CU8>
                                                          : k_channelize_resample;
  return launch_bank(kernel, "k_channelize_resample", a, rows * a.gpr, a.threads, lds, device, stream, W);
}

}  // namespace
}  // namespace lora

using lora::set_last_error;

extern "C" {

int64_t lora_resample_outputs(int64_t row_len, int64_t ntaps, int64_t interp, int64_t decim) {
  if (row_len < 0 || ntaps < 1 || interp < 1 || decim < 1)
    return set_last_error(LORA_EINVAL, "row_len must be >= 0, ntaps >= 1, interp >= 1 and decim >= 1");
  if (row_len > INT64_MAX / interp) return set_last_error(LORA_EINVAL, "row_len * interp overflows");
  return lora::resample_outputs(row_len, ntaps, interp, decim);
}

int64_t lora_resample_channelize_batch(const float* iq, int64_t rows, int64_t row_len, int64_t row_stride,
                                       int64_t first_sample, const float* taps, int64_t ntaps, int64_t interp,
                                       int64_t decim, const float* nco, int64_t period, const int32_t* steps,
                                       int64_t channels, float* out, int64_t out_stride, int device,
                                       void* stream) {
  return lora::resample_channelize(iq, lora::kIqCf32, 0.0f, rows, row_len, row_stride, first_sample, taps, ntaps,
                                   interp, decim, nco, period, steps, channels, out, out_stride, device, stream);
}

int64_t lora_resample_channelize_raw_batch(const void* iq, int format, float scale, int64_t rows, int64_t row_len,
                                           int64_t row_stride, int64_t first_sample, const float* taps,
                                           int64_t ntaps, int64_t interp, int64_t decim, const float* nco,
                                           int64_t period, const int32_t* steps, int64_t channels, float* out,
                                           int64_t out_stride, int device, void* stream) {
  if (const char* bad = lora::raw_format_error(iq, format)) return set_last_error(LORA_EINVAL, bad);
  return lora::resample_channelize(iq, format, scale, rows, row_len, row_stride, first_sample, taps, ntaps, interp,
                                   decim, nco, period, steps, channels, out, out_stride, device, stream);
}

}  // extern "C"
