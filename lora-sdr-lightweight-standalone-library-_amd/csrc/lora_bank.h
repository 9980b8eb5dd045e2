// lora_bank.h — what the three filter banks share: the down-converter banks
// (csrc/lora_channelize.hip, csrc/lora_resample.hip) and the synthesis bank (csrc/lora_synth.hip).
//
// All three.  A channel's oscillator is a table of `period` <= 4096 entries and a step per channel;
// the steps reach the kernel reduced into 0 .. period-1 (bank_steps), and a position in the table
// is found with divmod, a 24-bit multiply and a reciprocal in place of a 64-bit modulo.  A launch
// is one workgroup per tile, `gpr` tiles per row, rows * gpr < 2^31 (grid_error); launch_bank
// makes the device current, launches and reports.  A call is refused before any HIP call, first
// rule first; the texts of the rules are below, once each, and every entry keeps its own order of
// them (tests/test_bank_error_texts.py pins text and order).
//
// The down-converter banks.  Both mix every sample of a tile once per channel into LDS by phase
// (MixStage): sample s at [s % decim][s / decim], a row of pitch ps per phase, one channel
// channel_entries() entries after the other.  channel_geometry picks the tile and the channels per
// pass from `reach`, the samples an output reaches from its first one on: ntaps in the integer
// bank, max(off + K) over the residues in the rational one.  Their common argument rules come in
// two groups round the bank's own (ntaps, interp, decim): down_args_error in front of them,
// down_shape_error after them, then down_output_error once the outputs per row are known.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "lora_device.h"
#include "lora_internal.h"
#include "lora_iq_format.h"

#pragma clang fp contract(off)

namespace lora {

constexpr int kMaxPeriod = 4096, kMaxChannels = 32;
// the down-converter banks' tile and the mixed samples a workgroup holds (64 KiB)
constexpr int kMaxTile = 64, kMinTile = 8;
constexpr int kLdsSamples = 8192;

// ---- device ---------------------------------------------------------------------------------

// a / d and a % d for 0 <= a < 2^24, d <= 4096 and a / d < 2^13, inv = 1.0f / d: the product is
// within a / d * 2^-23 < 1 of the quotient, so its truncation is off by at most one either way
// (the products here are of 24-bit operands: __umul24 runs at full rate, a 32-bit multiply at a
// quarter of it)
__device__ __forceinline__ void divmod(unsigned a, unsigned d, float inv, unsigned& q, unsigned& r) {
  q = (unsigned)((float)a * inv);
  int rr = (int)a - (int)__umul24(q, d);
  if (rr < 0) {
    rr += (int)d;
    --q;
  } else if (rr >= (int)d) {
    rr -= (int)d;
    ++q;
  }
  r = (unsigned)rr;
}

// LDS entries of one channel: decim phase rows of `tile` outputs plus the reach
__host__ __device__ constexpr int channel_entries(int tile, int reach, int decim) {
  return decim * (tile + (reach - 1) / decim);
}

// The mix stage of a pass, as the `mix` that load_samples calls for every sample s of the tile:
// the sample times each oscillator of channels c0 .. c0 + nc - 1, to Z[c][s % decim][s / decim]
// (a channel `chs` entries).  p0 is the oscillator's position at the tile's first sample.  A is
// ChanArgs or ResArgs: decim, period, ps, steps, inv_decim, inv_period.  The members are references
// to the kernel's own variables, as a capturing lambda written in the kernel would hold them, and
// the kernel makes the load_samples call itself: with that the kernels compile to the instructions
// of such a lambda, to the byte; with copies as members, or with the call
// in a helper of its own, the compiler orders the scalar work round the FIR otherwise.
template <class A>
struct MixStage {
  const A& a;
  const cf* __restrict const& nco;
  v2f* const& Z;
  const unsigned& p0;
  const int &c0, &nc, &chs;
  __device__ __forceinline__ void operator()(int s, float xr, float xi) const {
    unsigned q, ph, u, p;
    divmod((unsigned)s, (unsigned)a.decim, a.inv_decim, q, ph);
    divmod(p0 + (unsigned)s, (unsigned)a.period, a.inv_period, u, p);
    v2f* dst = Z + ph * a.ps + q;
#pragma unroll 4
    for (int c = 0; c < nc; ++c) {
      unsigned m;
      divmod(__umul24((unsigned)a.steps[c0 + c], p), (unsigned)a.period, a.inv_period, u, m);
      const cf w = nco[m];
      v2f z;
      z.x = xr * w.re - xi * w.im;
      z.y = xr * w.im + xi * w.re;
      dst[c * chs] = z;
    }
  }
};

// ---- host: the rules, nullptr or the refusal's text --------------------------------------------

inline const char* period_channels_error(int64_t period, int64_t channels) {
  if (period < 1 || period > kMaxPeriod) return "period must be in 1..4096";
  if (channels < 1 || channels > kMaxChannels) return "channels must be in 1..32";
  return nullptr;
}

// rows * gpr < 2^31, compared through the quotient so that nothing overflows
inline const char* grid_error(int64_t rows, int64_t gpr) {
  return rows > 0 && gpr > 0 && rows > ((int64_t(1) << 31) - 1) / gpr ? "batch too large" : nullptr;
}

inline const char* down_args_error(const float* taps, const float* nco, const int32_t* steps, const float* out,
                                   int64_t rows, int64_t row_len, int64_t row_stride, int64_t out_stride,
                                   int64_t first_sample) {
  if (!taps || !nco || !steps || !out) return "null taps / nco / steps / out";
  if (rows < 0 || row_len < 0 || row_stride < 0 || out_stride < 0 || first_sample < 0)
    return "negative rows / row_len / row_stride / out_stride / first_sample";
  return nullptr;
}

inline const char* down_shape_error(int64_t period, int64_t channels, int64_t rows, int64_t row_len,
                                    int64_t row_stride) {
  if (const char* bad = period_channels_error(period, channels)) return bad;
  if (row_len >= (int64_t(1) << 31)) return "row_len must be < 2^31";
  if (rows > 1 && row_stride < row_len) return "row_stride smaller than row_len";
  return nullptr;
}

inline const char* down_output_error(int64_t out_stride, int64_t W, int64_t rows, int64_t gpr) {
  if (out_stride < W) return "out_stride smaller than outputs per row";
  return grid_error(rows, gpr);
}

// ---- host: geometry and launch ---------------------------------------------------------------

// Outputs (of one residue) per workgroup and channels per pass of a down-converter bank: the
// largest tile of 64, 32, 16, 8 at which all channels fit the LDS; at 8 whatever fits
inline void channel_geometry(int reach, int decim, int channels, int& tile, int& cg) {
  tile = kMaxTile;
  while (tile > kMinTile && (int64_t)channels * channel_entries(tile, reach, decim) > kLdsSamples) tile >>= 1;
  cg = kLdsSamples / channel_entries(tile, reach, decim);
  if (cg > channels) cg = channels;
}

// steps[c] mod period, each in 0 .. period-1
inline void bank_steps(const int32_t* steps, int channels, int64_t period, int* out) {
  for (int c = 0; c < channels; ++c) {
    const int64_t k = (int64_t)steps[c] % period;
    out[c] = (int)(k < 0 ? k + period : k);
  }
}

// One bank kernel, `grid` workgroups of `threads` lanes on `stream` of `device`: `ret`, or LORA_EIO
// with a text that names the step
template <class A>
int64_t launch_bank(void (*kernel)(A), const char* name, const A& a, int64_t grid, int threads, size_t lds,
                    int device, void* stream, int64_t ret) {
  DeviceGuard guard(device);
  if (guard.err != hipSuccess) return hip_error((std::string(name) + " device").c_str(), guard.err);
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3((unsigned)threads), lds, static_cast<hipStream_t>(stream), a);
  const hipError_t e = hipGetLastError();
  return e != hipSuccess ? hip_error(name, e) : ret;
}

}  // namespace lora
