// lora_channelize.hip — the digital down-converter bank (lora_channelize_batch).
//
// One wideband row in, `channels` rows at the demodulator's rate out: every sample is mixed
// with each channel's oscillator (a table the caller supplies), then a real FIR of `ntaps`
// taps is evaluated every `decim` samples.  The arithmetic is the header's, operation for
// operation: fp32, one rounding each, no contraction, the taps accumulated in order from
// +0.0f.  The reference has no channelizer; the definition is this library's own
// (tests/channel_checker.py restates it in numpy and the GPU tests compare bits).
//
// A workgroup owns `tile` consecutive outputs of every channel of one row.  It reads the
// (tile-1)*decim + ntaps samples they cover once, with 16-byte loads, and mixes each sample
// once per channel into LDS.  The mixed samples of a channel are kept by phase: sample s sits
// at [s % decim][s / decim], a row of pitch ps = tile + (ntaps-1)/decim per phase, so that the
// FIR's read of tap j for consecutive outputs (samples decim apart) is a read of consecutive
// LDS entries.  The FIR runs from LDS, one output index per lane and two channels per lane at
// a time; the taps are loaded 64 at a time, one per lane, and handed round by readlane.
// tile is 64 where all channels fit the 64 KiB of LDS at once (channel_geometry, csrc/lora_bank.h);
// otherwise it shrinks to 32, 16 or 8, and if the channels still do not fit they are taken in
// passes of `cg`, each pass re-reading the tile's samples (the ABI's extremes, 32 channels of
// 512 taps at decim 64, run that way).  The mix stage, the oscillator's arithmetic, the geometry's
// search and the argument rules are shared with the other banks: csrc/lora_bank.h.
//
// The kernel is a template over the sample format (csrc/lora_iq_format.h): complex64 for
// lora_channelize_batch, cs16, cs8 and cu8 for lora_channelize_raw_batch, whose integer samples
// become fp32 in the load in front of the mixing and are otherwise the same kernel's.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/lora_mi355x.h"
#include "lora_bank.h"

#pragma clang fp contract(off)

namespace lora {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxTaps = 512, kMaxDecim = 64;

struct ChanArgs {
  const void* iq;  // samples of the kernel's format
  const float* taps;
  const cf* nco;
  cf* out;
  int64_t row_stride, out_stride, W, gpr;
  int ntaps, decim, period, channels;
  int first_mod;  // first_sample mod period
  int tile, lg_tile, ps, cg;
  float inv_decim, inv_period;
  int steps[kMaxChannels];  // each in 0 .. period-1
  float scale;              // of an integer format's samples
};

template <int F>
__global__ void __launch_bounds__(kThreads) k_channelize(ChanArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  v2f* Z = reinterpret_cast<v2f*>(smem);  // [cg][decim][ps]
  const int tid = threadIdx.x;
  const int64_t row = (int64_t)blockIdx.x / a.gpr;
  const int64_t t0 = ((int64_t)blockIdx.x - row * a.gpr) * a.tile;
  const int nv = a.W - t0 < a.tile ? (int)(a.W - t0) : a.tile;  // >= 1
  // the tile's first sample and how many it covers; the last output's window ends inside the
  // row ((W-1)*decim + ntaps <= row_len), so nothing below reads past it
  const int64_t n0 = t0 * a.decim;  // < row_len < 2^31
  const int cnt = (nv - 1) * a.decim + a.ntaps;
  const int chs = channel_entries(a.tile, a.ntaps, a.decim);
  // the oscillator's position at the tile's first sample: (first_sample + n0) mod period
  const unsigned p0 = ((unsigned)a.first_mod + (unsigned)n0 % (unsigned)a.period) % (unsigned)a.period;
  const int tl = tid & (a.tile - 1), cl = tid >> a.lg_tile, ncl = kThreads >> a.lg_tile;
  const float* __restrict__ taps = a.taps;
  const cf* __restrict__ nco = a.nco;

  for (int c0 = 0; c0 < a.channels; c0 += a.cg) {
    const int nc = a.channels - c0 < a.cg ? a.channels - c0 : a.cg;
    if (c0) __syncthreads();  // the previous pass's FIR has read Z

    // every sample of the tile, mixed for the pass's channels.  Pairs of samples on the grid of a
    // pair's size (16 bytes of complex64); a pair that hangs over either end is loaded singly
    const MixStage<ChanArgs> mix{a, nco, Z, p0, c0, nc, chs};
    load_samples<F>(a.iq, row * a.row_stride + n0, cnt, a.scale, tid, kThreads, mix);
    __syncthreads();

    // output t0 + tl of channels c and c + ncl: tap j meets sample tl * decim + j, entry
    // [j % decim][tl + j / decim].  Every lane of the workgroup runs the loop, because every
    // lane's tap is read by readlane; a lane with no output (tl >= nv, or no channel left)
    // works on entries inside Z that belong to others or were never written, and stores nothing.
    for (int cb = 0; cb < nc; cb += 2 * ncl) {
      const int c = cb + cl;
      const bool one = tl < nv && c < nc, two = tl < nv && c + ncl < nc;
      const v2f* z0 = Z + (c < nc ? c : 0) * chs + tl;
      const v2f* z1 = Z + (c + ncl < nc ? c + ncl : 0) * chs + tl;
      v2f y0 = {0.0f, 0.0f}, y1 = {0.0f, 0.0f};
      // 64 taps at a time, one per lane, handed round by readlane; `at` walks the phase rows
      int ph = 0, at = 0;
      for (int jb = 0; jb < a.ntaps; jb += 64) {
        const int n = a.ntaps - jb < 64 ? a.ntaps - jb : 64;
        const int hv = (tid & 63) < n ? __float_as_int(taps[jb + (tid & 63)]) : 0;
        for (int jj = 0; jj < n; ++jj) {
          const float h = __int_as_float(__builtin_amdgcn_readlane(hv, jj));
          y0 = y0 + h * z0[at];
          y1 = y1 + h * z1[at];
          at += a.ps;
          if (++ph == a.decim) {
            ph = 0;
            at -= a.decim * a.ps - 1;
          }
        }
      }
      v2f* o = reinterpret_cast<v2f*>(a.out) + ((row * a.channels + c0 + c) * a.out_stride + t0 + tl);
      if (one) *o = y0;
      if (two) o[(int64_t)ncl * a.out_stride] = y1;
    }
  }
}

int64_t channel_outputs(int64_t row_len, int64_t ntaps, int64_t decim) {
  return row_len < ntaps ? 0 : (row_len - ntaps) / decim + 1;
}

// Both entries: `format` is kIqCf32 for lora_channelize_batch, else a checked LORA_IQ_*
int64_t channelize(const void* iq, int format, float scale, int64_t rows, int64_t row_len, int64_t row_stride,
                   int64_t first_sample, const float* taps, int64_t ntaps, int64_t decim, const float* nco,
                   int64_t period, const int32_t* steps, int64_t channels, float* out, int64_t out_stride,
                   int device, void* stream) {
  if (const char* bad = down_args_error(taps, nco, steps, out, rows, row_len, row_stride, out_stride, first_sample))
    return set_last_error(LORA_EINVAL, bad);
  if (ntaps < 1 || ntaps > kMaxTaps) return set_last_error(LORA_EINVAL, "ntaps must be in 1..512");
  if (decim < 1 || decim > kMaxDecim) return set_last_error(LORA_EINVAL, "decim must be in 1..64");
  if (const char* bad = down_shape_error(period, channels, rows, row_len, row_stride))
    return set_last_error(LORA_EINVAL, bad);
  const int64_t W = channel_outputs(row_len, ntaps, decim);
  ChanArgs a{};
  channel_geometry((int)ntaps, (int)decim, (int)channels, a.tile, a.cg);
  a.W = W;
  a.gpr = (W + a.tile - 1) / a.tile;
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
  a.decim = (int)decim;
  a.period = (int)period;
  a.channels = (int)channels;
  a.first_mod = (int)(first_sample % period);
  for (a.lg_tile = 0; (1 << a.lg_tile) < a.tile; ++a.lg_tile) {
  }
  a.ps = a.tile + (a.ntaps - 1) / a.decim;
  a.inv_decim = 1.0f / (float)a.decim;
  a.inv_period = 1.0f / (float)a.period;
  bank_steps(steps, a.channels, period, a.steps);
  const size_t lds = (size_t)a.cg * channel_entries(a.tile, a.ntaps, a.decim) * sizeof(cf);
  void (*const kernel)(ChanArgs) = format == LORA_IQ_CS16  ? k_channelize<LORA_IQ_CS16>
                                   : format == LORA_IQ_CS8 ? k_channelize<LORA_IQ_CS8>
                                   : format == LORA_IQ_CU8 ? k_channelize<LORA_IQ_CU8>
                                                           : k_channelize<kIqCf32>;
  return launch_bank(kernel, "k_channelize", a, rows * a.gpr, kThreads, lds, device, stream, W);
}

}  // namespace
}  // namespace lora

using lora::set_last_error;

extern "C" {

int64_t lora_channelize_outputs(int64_t row_len, int64_t ntaps, int64_t decim) {
  if (row_len < 0 || ntaps < 1 || decim < 1)
    return set_last_error(LORA_EINVAL, "row_len must be >= 0, ntaps >= 1 and decim >= 1");
  return lora::channel_outputs(row_len, ntaps, decim);
}

int64_t lora_channelize_batch(const float* iq, int64_t rows, int64_t row_len, int64_t row_stride,
                              int64_t first_sample, const float* taps, int64_t ntaps, int64_t decim,
                              const float* nco, int64_t period, const int32_t* steps, int64_t channels,
                              float* out, int64_t out_stride, int device, void* stream) {
  return lora::channelize(iq, lora::kIqCf32, 0.0f, rows, row_len, row_stride, first_sample, taps, ntaps, decim, nco,
                          period, steps, channels, out, out_stride, device, stream);
}

int64_t lora_channelize_raw_batch(const void* iq, int format, float scale, int64_t rows, int64_t row_len,
                                  int64_t row_stride, int64_t first_sample, const float* taps, int64_t ntaps,
                                  int64_t decim, const float* nco, int64_t period, const int32_t* steps,
                                  int64_t channels, float* out, int64_t out_stride, int device, void* stream) {
  if (const char* bad = lora::raw_format_error(iq, format)) return set_last_error(LORA_EINVAL, bad);
  return lora::channelize(iq, format, scale, rows, row_len, row_stride, first_sample, taps, ntaps, decim, nco, period,
                          steps, channels, out, out_stride, device, stream);
}

}  // extern "C"
