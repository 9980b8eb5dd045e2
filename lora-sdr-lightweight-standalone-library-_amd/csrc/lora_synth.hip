// lora_synth.hip — the synthesis bank (lora_synthesize_batch, lora_synthesize_raw_batch): the
// inverse of the down-converter banks.  `channels` streams at the modulator's rate in, one
// wideband row out: every channel is scaled by its gain, interpolated by `interp` with a real
// polyphase FIR, mixed up by its oscillator (a table the caller supplies) and the channels are
// summed in order.  The arithmetic is the header's, operation for operation: fp32, one rounding
// each, no contraction, every accumulator from +0.0f.  The reference has no synthesiser; the
// definition is this library's own (tests/synth_checker.py restates it in numpy and the GPU
// tests compare bits).
//
// A workgroup of 256 lanes owns kTile = 1024 consecutive outputs of one row; lane l owns outputs
// l, l + 256, l + 512 and l + 768 of the tile, so the lanes of a wave work on consecutive
// outputs: `interp` neighbours read the same LDS entry of a channel (a broadcast) and lanes
// `interp` apart the same tap, and neither read has a bank conflict at any `interp`.  The
// tile's (kTile - 1) / interp + P (or one more) gain-scaled samples of every channel are staged
// in LDS once, beside the taps; where all channels do not fit the 64 KiB they are taken in
// passes of `cg` in channel order, the four sums of a lane staying in its registers across the
// passes.  K is P or P - 1 for every phase, so the tap loop runs P - 1 uniform steps and one
// predicated step.  The oscillator's position is found per output once, by the bank's 24-bit
// multiply and reciprocal (no 64-bit modulo), and per channel the same way (divmod; it, the
// steps' reduction, the grid's limit and the launch are the banks' own: csrc/lora_bank.h).
//
// The kernel is a template over the output format (csrc/lora_iq_format.h): complex64, or cs16,
// cs8, cu8 made by iq_store_code.  A tile's samples are put in LDS at the offset their global
// address has in a 16-byte line and leave with 16-byte stores; the samples of a line that the
// row's first or last output cuts are stored singly.  So `out` need only be aligned to one
// sample and the bits do not depend on the alignment.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/lora_mi355x.h"
#include "lora_bank.h"

#pragma clang fp contract(off)

namespace lora {
namespace {

constexpr int kThreads = 256;
constexpr int kPerLane = 4;
constexpr int kTile = kThreads * kPerLane;
constexpr int kMaxTaps = 512, kMaxInterp = 64;
constexpr int kLdsBytes = 65536;

struct SynthArgs {
  const cf* in;
  const float* taps;
  const cf* nco;
  void* out;  // samples of the kernel's format
  int64_t in_stride, out_stride, W, gpr;
  int ntaps, interp, period, channels;
  int P;          // ceil(ntaps / interp)
  int first_mod;  // first_sample mod period
  int pitch, cg;  // LDS entries per channel (even), channels per pass
  float inv_interp, inv_period, inv_scale;
  int steps[kMaxChannels];  // each in 0 .. period-1
  float gains[kMaxChannels];
};

// LDS entries a tile can need of one channel, rounded up to even: its outputs span at most
// (kTile - 1) / interp + 2 values of q, and each reaches P - 1 samples further
__host__ __device__ constexpr int synth_pitch(int P, int interp) {
  return ((kTile - 1) / interp + 1 + P + 1) & ~1;
}
__host__ __device__ constexpr int out_buf_bytes(int format) { return kTile * iq_sample_bytes(format) + 16; }

template <int F>
__global__ void __launch_bounds__(kThreads) k_synthesize(SynthArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int SB = iq_sample_bytes(F);
  v2f* A = reinterpret_cast<v2f*>(smem);                  // [cg][pitch], gain-scaled samples
  unsigned char* obuf = smem + (size_t)a.cg * a.pitch * 8;  // the tile's stored samples
  float* H = reinterpret_cast<float*>(obuf + out_buf_bytes(F));
  const int tid = threadIdx.x;
  const int64_t row = (int64_t)blockIdx.x / a.gpr;
  const int64_t t0 = ((int64_t)blockIdx.x - row * a.gpr) * kTile;  // < W < 2^31
  const int nv = a.W - t0 < kTile ? (int)(a.W - t0) : kTile;       // >= 1
  const unsigned U = (unsigned)a.interp, P = (unsigned)a.P;
  const unsigned q0 = (unsigned)t0 / U, r0 = (unsigned)t0 % U;
  // samples q0 .. q0 + nin - 1 of each channel: the last output's q plus its P - 1 further ones;
  // q <= chan_len - P for every output below W, so the last one is inside the stream
  const int nin = (int)(((unsigned)t0 + (unsigned)nv - 1) / U - q0 + P);
  const unsigned pos0 = ((unsigned)a.first_mod + (unsigned)t0 % (unsigned)a.period) % (unsigned)a.period;
  const float* __restrict__ taps = a.taps;
  const cf* __restrict__ nco = a.nco;

  for (int j = tid; j < a.ntaps; j += kThreads) H[j] = taps[j];

  // this lane's outputs t0 + off[v]; a lane past the tile's end repeats the last output and
  // stores nothing
  bool valid[kPerLane], full[kPerLane];
  unsigned pos[kPerLane];
  int hp[kPerLane], ap[kPerLane];
#pragma unroll
  for (int v = 0; v < kPerLane; ++v) {
    const int o = v * kThreads + tid;
    valid[v] = o < nv;
    const unsigned off = valid[v] ? (unsigned)o : (unsigned)(nv - 1);
    unsigned q, p, u;
    divmod(r0 + off, U, a.inv_interp, q, p);
    divmod(pos0 + off, (unsigned)a.period, a.inv_period, u, pos[v]);
    hp[v] = (int)p;
    ap[v] = (int)(q + P - 1);
    // K == P where tap p + (P-1)*interp exists, else P - 1
    full[v] = p + (P - 1) * U < (unsigned)a.ntaps;
  }

  float yr[kPerLane], yi[kPerLane];
#pragma unroll
  for (int v = 0; v < kPerLane; ++v) yr[v] = yi[v] = 0.0f;

  const float inv_nin = 1.0f / (float)nin;
  for (int c0 = 0; c0 < a.channels; c0 += a.cg) {
    const int nc = a.channels - c0 < a.cg ? a.channels - c0 : a.cg;
    if (c0) __syncthreads();  // the previous pass's sums have read A
    const cf* src = a.in + ((row * a.channels + c0) * a.in_stride + q0);
    for (int e = tid; e < nc * nin; e += kThreads) {
      unsigned c, j;
      divmod((unsigned)e, (unsigned)nin, inv_nin, c, j);
      const cf x = src[(int64_t)c * a.in_stride + j];
      const float g = a.gains[c0 + c];
      v2f s;
      s.x = g * x.re;
      s.y = g * x.im;
      A[c * a.pitch + j] = s;
    }
    __syncthreads();

    for (int c = 0; c < nc; ++c) {
      const v2f* Ac = A + c * a.pitch;
      float sr[kPerLane], si[kPerLane];
#pragma unroll
      for (int v = 0; v < kPerLane; ++v) sr[v] = si[v] = 0.0f;
      int hoff = 0;
      for (unsigned i = 0; i + 1 < P; ++i, hoff += (int)U) {
#pragma unroll
        for (int v = 0; v < kPerLane; ++v) {
          const float h = H[hp[v] + hoff];
          const v2f z = Ac[ap[v] - (int)i];
          sr[v] = sr[v] + h * z.x;
          si[v] = si[v] + h * z.y;
        }
      }
      const unsigned kc = (unsigned)a.steps[c0 + c];
#pragma unroll
      for (int v = 0; v < kPerLane; ++v) {
        if (full[v]) {
          const float h = H[hp[v] + hoff];
          const v2f z = Ac[ap[v] - (int)(P - 1)];
          sr[v] = sr[v] + h * z.x;
          si[v] = si[v] + h * z.y;
        }
        unsigned u, m;
        divmod(__umul24(kc, pos[v]), (unsigned)a.period, a.inv_period, u, m);
        const cf w = nco[m];
        const float zr = sr[v] * w.re - si[v] * w.im;
        const float zi = sr[v] * w.im + si[v] * w.re;
        yr[v] = yr[v] + zr;
        yi[v] = yi[v] + zi;
      }
    }
  }

  // the tile's samples in the output's format, at the offset of their address in its 16-byte line
  unsigned char* g = static_cast<unsigned char*>(a.out) + (row * a.out_stride + t0) * SB;
  const int mis = (int)(reinterpret_cast<uintptr_t>(g) & 15);  // a multiple of SB
#pragma unroll
  for (int v = 0; v < kPerLane; ++v) {
    if (!valid[v]) continue;
    unsigned char* o = obuf + mis + (v * kThreads + tid) * SB;
    if constexpr (F == kIqCf32) {
      v2f y;
      y.x = yr[v];
      y.y = yi[v];
      *reinterpret_cast<v2f*>(o) = y;
    } else {
      const unsigned w = iq_pack<F>(iq_store_code<F>(yr[v], a.inv_scale), iq_store_code<F>(yi[v], a.inv_scale));
      if constexpr (SB == 4)
        *reinterpret_cast<unsigned*>(o) = w;
      else
        *reinterpret_cast<unsigned short*>(o) = (unsigned short)w;
    }
  }
  __syncthreads();
  const int end = mis + nv * SB;
  for (int k = tid; k * 16 < end; k += kThreads) {
    const int lo = k * 16, hi = lo + 16;
    if (lo >= mis && hi <= end) {
      *reinterpret_cast<uint4*>(g - mis + lo) = *reinterpret_cast<const uint4*>(obuf + lo);
    } else {
      const int b0 = lo < mis ? mis : lo, b1 = hi < end ? hi : end;
      for (int b = b0; b < b1; b += SB) {
        if constexpr (SB == 8)
          *reinterpret_cast<v2f*>(g - mis + b) = *reinterpret_cast<const v2f*>(obuf + b);
        else if constexpr (SB == 4)
          *reinterpret_cast<unsigned*>(g - mis + b) = *reinterpret_cast<const unsigned*>(obuf + b);
        else
          *reinterpret_cast<unsigned short*>(g - mis + b) = *reinterpret_cast<const unsigned short*>(obuf + b);
      }
    }
  }
}

int64_t synth_outputs(int64_t chan_len, int64_t ntaps, int64_t interp) {
  const int64_t P = (ntaps + interp - 1) / interp;
  return chan_len < P ? 0 : (chan_len - P + 1) * interp;
}

// Both entries: `format` is kIqCf32 for lora_synthesize_batch, else a checked LORA_IQ_*
int64_t synthesize(const float* in, int64_t rows, int64_t chan_len, int64_t in_stride, int64_t first_sample,
                   const float* taps, int64_t ntaps, int64_t interp, const float* nco, int64_t period,
                   const int32_t* steps, const float* gains, int64_t channels, void* out, int format,
                   float inv_scale, int64_t out_stride, int device, void* stream) {
  if (rows < 0 || chan_len < 0 || in_stride < 0 || out_stride < 0 || first_sample < 0)
    return set_last_error(LORA_EINVAL, "negative rows / chan_len / in_stride / out_stride / first_sample");
  if (interp < 1 || interp > kMaxInterp) return set_last_error(LORA_EINVAL, "interp must be in 1..64");
  if (ntaps < 1 || ntaps > kMaxTaps) return set_last_error(LORA_EINVAL, "ntaps must be in 1..512");
  if (const char* bad = period_channels_error(period, channels)) return set_last_error(LORA_EINVAL, bad);
  if (chan_len >= (int64_t(1) << 31) || chan_len * interp >= (int64_t(1) << 31))
    return set_last_error(LORA_EINVAL, "chan_len * interp must be < 2^31");
  if (rows * channels > 1 && in_stride < chan_len)
    return set_last_error(LORA_EINVAL, "in_stride smaller than chan_len");
  const int64_t W = synth_outputs(chan_len, ntaps, interp);
  if (rows > 1 && out_stride < W) return set_last_error(LORA_EINVAL, "out_stride smaller than outputs per row");
  if (reinterpret_cast<uintptr_t>(out) % (uintptr_t)iq_sample_bytes(format))
    return set_last_error(LORA_EINVAL, "out is not aligned to one sample");
  SynthArgs a{};
  a.W = W;
  a.gpr = (W + kTile - 1) / kTile;
  if (const char* bad = grid_error(rows, a.gpr)) return set_last_error(LORA_EINVAL, bad);
  if (rows == 0 || W == 0) return W;
  if (!in || !taps || !nco || !steps || !gains || !out)
    return set_last_error(LORA_EINVAL, "null in / taps / nco / steps / gains / out");
  a.in = reinterpret_cast<const cf*>(in);
  a.taps = taps;
  a.nco = reinterpret_cast<const cf*>(nco);
  a.out = out;
  a.in_stride = in_stride;
  a.out_stride = out_stride;
  a.ntaps = (int)ntaps;
  a.interp = (int)interp;
  a.period = (int)period;
  a.channels = (int)channels;
  a.P = (int)((ntaps + interp - 1) / interp);
  a.first_mod = (int)(first_sample % period);
  a.inv_interp = 1.0f / (float)a.interp;
  a.inv_period = 1.0f / (float)a.period;
  a.inv_scale = inv_scale;
  bank_steps(steps, a.channels, period, a.steps);
  for (int c = 0; c < a.channels; ++c) a.gains[c] = gains[c];
  // what the 64 KiB leave for samples after the taps and the tile's stored form: at least 4
  // channels per pass (a channel takes at most 1536 entries)
  a.pitch = synth_pitch(a.P, a.interp);
  const int fixed = out_buf_bytes(format) + a.ntaps * (int)sizeof(float);
  a.cg = (kLdsBytes - fixed) / (a.pitch * (int)sizeof(cf));
  if (a.cg > a.channels) a.cg = a.channels;
  const size_t lds = (size_t)a.cg * a.pitch * sizeof(cf) + fixed;
  void (*const kernel)(SynthArgs) = format == LORA_IQ_CS16  ? k_synthesize<LORA_IQ_CS16>
                                    : format == LORA_IQ_CS8 ? k_synthesize<LORA_IQ_CS8>
                                    : format == LORA_IQ_CU8 ? k_synthesize<LORA_IQ_CU8>
                                                            : k_synthesize<kIqCf32>;
  return launch_bank(kernel, "k_synthesize", a, rows * a.gpr, kThreads, lds, device, stream, W);
}

}  // namespace
}  // namespace lora

using lora::set_last_error;

extern "C" {

int64_t lora_synthesize_outputs(int64_t chan_len, int64_t ntaps, int64_t interp) {
  if (chan_len < 0 || ntaps < 1 || interp < 1 || chan_len > INT64_MAX / interp)
    return set_last_error(LORA_EINVAL, "chan_len must be >= 0, ntaps >= 1, interp >= 1 and chan_len * interp in 64 bits");
  return lora::synth_outputs(chan_len, ntaps, interp);
}

int64_t lora_synthesize_batch(const float* in, int64_t rows, int64_t chan_len, int64_t in_stride,
                              int64_t first_sample, const float* taps, int64_t ntaps, int64_t interp,
                              const float* nco, int64_t period, const int32_t* steps, const float* gains,
                              int64_t channels, float* out, int64_t out_stride, int device, void* stream) {
  return lora::synthesize(in, rows, chan_len, in_stride, first_sample, taps, ntaps, interp, nco, period, steps, gains,
                          channels, out, lora::kIqCf32, 0.0f, out_stride, device, stream);
}

int64_t lora_synthesize_raw_batch(const float* in, int64_t rows, int64_t chan_len, int64_t in_stride,
                                  int64_t first_sample, const float* taps, int64_t ntaps, int64_t interp,
                                  const float* nco, int64_t period, const int32_t* steps, const float* gains,
                                  int64_t channels, void* out, int format, float inv_scale, int64_t out_stride,
                                  int device, void* stream) {
  if (format != LORA_IQ_CS16 && format != LORA_IQ_CS8 && format != LORA_IQ_CU8)
    return set_last_error(LORA_EINVAL, "format must be LORA_IQ_CS16, LORA_IQ_CS8 or LORA_IQ_CU8");
  return lora::synthesize(in, rows, chan_len, in_stride, first_sample, taps, ntaps, interp, nco, period, steps, gains,
                          channels, out, format, inv_scale, out_stride, device, stream);
}

}  // extern "C"
