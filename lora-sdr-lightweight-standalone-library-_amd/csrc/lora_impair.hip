// lora_impair.hip — the channel impairment stage (lora_impair_batch, lora_impair_raw_batch): what
// stands between the synthesis bank and the down-converter banks.  Rows of complex64 in, the same
// rows out with a gain, a carrier offset (a 32-bit phase accumulator) and counter-based white
// Gaussian noise (Philox4x32-10, Box-Muller) applied, read once and written once, as complex64 or
// as cs16 / cs8 / cu8 codes.  The arithmetic is the header's, operation for operation: fp32, one
// rounding each, no contraction; the sines, cosines and logarithms are glibc's to the bit
// (csrc/lora_libm.h).  The reference's channel is three lines of host code in its AWGN test; the
// definition is this library's own (tests/impair_checker.py restates it in numpy and the GPU
// tests compare bits).
//
// A sample's value depends on (seed, first_row + r, first_sample + t) and its row's parameters
// alone, so nothing below - the tile, the pairing, which lane holds a sample - can show in the
// bits.
//
// A workgroup of 256 lanes owns kTile = 1024 consecutive samples of one row and no LDS.  A lane
// takes two samples per round: pair q holds samples 2q - mis and 2q + 1 - mis of the tile, mis
// the offset of the tile's first OUTPUT sample on the grid of two stored samples, so that a pair
// leaves with one store of 16 bytes of complex64 (8 of cs16, 4 of an 8-bit format) and
// consecutive lanes store consecutive addresses; it arrives with one 16-byte load where the
// input lies on the same grid (always when out == in) and two 8-byte loads otherwise.  The one
// sample that may hang over either end of the tile goes singly.  The lane that loads a sample
// stores it, which is what makes out == in safe.
//
// A Philox block gives the noise of samples 2b and 2b + 1.  Whether a lane's pair is such an
// even/odd pair is the same for the whole workgroup: then one block serves both samples, else
// the lane computes the two blocks it needs a half of.  The lane's two rotations and two noise
// phases go through one interleaved four-way sincos (lm_sincosf_fast_k), the two logarithms
// through a two-way one.  The row's parameters are uniform over the workgroup: scalar loads.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/lora_mi355x.h"
#include "lora_bank.h"
#include "lora_libm.h"

#pragma clang fp contract(off)

namespace lora {
namespace {

constexpr int kThreads = 256;
constexpr int kTile = 1024;
constexpr float kWordToRad = 0x1.921fb6p-30f;  // fp32 pi * 2^-31: a signed 32-bit word to (-pi, pi]

struct ImpairArgs {
  const cf* in;  // nullptr: noise-only rows
  void* out;     // samples of the kernel's format
  const float* gain;
  const int32_t* fcw;
  const int32_t* phase;
  const float* sigma;
  int64_t in_stride, out_stride, row_len, gpr;
  uint64_t first_sample, first_row;
  uint32_t key0, key1;
  float inv_scale;
};

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                              uint32_t k1, uint32_t (&w)[4]) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0;
    c1 = l1;
    c2 = h0 ^ c3 ^ k1;
    c3 = l0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  w[0] = c0;
  w[1] = c1;
  w[2] = c2;
  w[3] = c3;
}

template <int F>
__global__ void __launch_bounds__(kThreads) k_impair(ImpairArgs a) {
  constexpr int SB = iq_sample_bytes(F);
  const int tid = threadIdx.x;
  const int64_t row = (int64_t)blockIdx.x / a.gpr;
  const int64_t t0 = ((int64_t)blockIdx.x - row * a.gpr) * kTile;
  const int nv = a.row_len - t0 < kTile ? (int)(a.row_len - t0) : kTile;  // >= 1

  const bool has_in = a.in != nullptr;
  const bool do_gain = has_in && a.gain != nullptr;
  const bool do_rot = has_in && (a.fcw != nullptr || a.phase != nullptr);
  const bool do_noise = a.sigma != nullptr;
  const float g = do_gain ? a.gain[row] : 0.0f;
  const uint32_t fcw = do_rot && a.fcw ? (uint32_t)a.fcw[row] : 0u;
  const uint32_t ph0 = do_rot && a.phase ? (uint32_t)a.phase[row] : 0u;
  const float sg = do_noise ? a.sigma[row] : 0.0f;
  const uint64_t R = a.first_row + (uint64_t)row;
  // The key in vector registers: as scalars the ten rounds' keys are computed once and held for
  // the whole loop, twenty scalar registers that the kernel does not have to spare (it spilled
  // two); as vector values they are two adds per round beside the round's four multiplies.
  uint32_t key0 = a.key0, key1 = a.key1;
  asm volatile("" : "+v"(key0), "+v"(key1));
  const uint64_t n0 = a.first_sample + (uint64_t)t0;

  unsigned char* o = static_cast<unsigned char*>(a.out) + (row * a.out_stride + t0) * SB;
  const cf* x = has_in ? a.in + (row * a.in_stride + t0) : nullptr;
  const int mis = (int)((reinterpret_cast<uintptr_t>(o) / SB) & 1);
  // the input's pairs lie on the 16-byte grid too
  const bool in16 = (int)((reinterpret_cast<uintptr_t>(x) >> 3) & 1) == mis;
  // the pairs are (even n, odd n): one Philox block each
  const bool shared = (((unsigned)n0 + (unsigned)mis) & 1u) == 0u;
  const int pairs = (nv + mis + 1) / 2;

  for (int q = tid; q < pairs; q += kThreads) {
    const int s0 = 2 * q - mis;
    const bool v0 = s0 >= 0, v1 = s0 + 1 < nv;
    const uint64_t nA = n0 + (uint64_t)(int64_t)s0;  // (of a sample that is not there: unused bits)
    float yr[2] = {0.0f, 0.0f}, yi[2] = {0.0f, 0.0f};
    if (has_in) {
      if (v0 && v1) {
        if (in16) {
          const float4 v = *reinterpret_cast<const float4*>(x + s0);
          yr[0] = v.x, yi[0] = v.y, yr[1] = v.z, yi[1] = v.w;
        } else {
          const cf u = x[s0], v = x[s0 + 1];
          yr[0] = u.re, yi[0] = u.im, yr[1] = v.re, yi[1] = v.im;
        }
      } else if (v0) {
        const cf u = x[s0];
        yr[0] = u.re, yi[0] = u.im;
      } else {
        const cf v = x[s0 + 1];
        yr[1] = v.re, yi[1] = v.im;
      }
    }
    if (do_gain) {
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        yr[k] = g * yr[k];
        yi[k] = g * yi[k];
      }
    }

    // the angles of this pair: two rotations, two noise phases
    float ang[4] = {0.0f, 0.0f, 0.0f, 0.0f}, sn[4], cs[4], u[2] = {0.5f, 0.5f};
    if (do_rot) {
      const uint32_t pA = ph0 + fcw * (uint32_t)nA;
      ang[0] = (float)(int32_t)pA * kWordToRad;
      ang[1] = (float)(int32_t)(pA + fcw) * kWordToRad;
    }
    if (do_noise) {
      const uint64_t b = nA >> 1;
      uint32_t w[4], wa[2], wb[2];
      philox4x32_10((uint32_t)b, (uint32_t)(b >> 32), (uint32_t)R, (uint32_t)(R >> 32), key0, key1, w);
      if (shared) {
        wa[0] = w[0], wa[1] = w[1], wb[0] = w[2], wb[1] = w[3];
      } else {
        wa[0] = w[2], wa[1] = w[3];
        const uint64_t b1 = (nA + 1) >> 1;  // (not b + 1: nA is 2^64 - 1 in front of sample 0)
        philox4x32_10((uint32_t)b1, (uint32_t)(b1 >> 32), (uint32_t)R, (uint32_t)(R >> 32), key0, key1, w);
        wb[0] = w[0], wb[1] = w[1];
      }
      u[0] = (float)(2u * (wa[0] >> 9) + 1u) * 0x1p-24f;
      u[1] = (float)(2u * (wb[0] >> 9) + 1u) * 0x1p-24f;
      ang[2] = (float)(int32_t)wa[1] * kWordToRad;
      ang[3] = (float)(int32_t)wb[1] * kWordToRad;
    }
    if (do_rot && do_noise) {
      lm_sincosf_fast_k<4>(ang, sn, cs);
    } else if (do_rot) {
      lm_sincosf_fast_k<2>(ang, sn, cs);
    } else if (do_noise) {
      lm_sincosf_fast_k<2>(ang + 2, sn + 2, cs + 2);
    }
    if (do_rot) {
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const float xr = yr[k], xi = yi[k];
        yr[k] = xr * cs[k] - xi * sn[k];
        yi[k] = xr * sn[k] + xi * cs[k];
      }
    }
    if (do_noise) {
      float lg[2];
      lm_logf_pos_k<2>(u, lg);
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const float rad = __builtin_sqrtf(-2.0f * lg[k]);  // correctly rounded (the compiler's IEEE lowering)
        const float amp = sg * rad;
        const float nr = amp * cs[2 + k], ni = amp * sn[2 + k];
        if (has_in) {
          yr[k] = yr[k] + nr;
          yi[k] = yi[k] + ni;
        } else {
          yr[k] = nr;
          yi[k] = ni;
        }
      }
    }

    unsigned char* dst = o + (int64_t)s0 * SB;  // on the grid of two stored samples
    if constexpr (F == kIqCf32) {
      if (v0 && v1) {
        float4 v;
        v.x = yr[0], v.y = yi[0], v.z = yr[1], v.w = yi[1];
        *reinterpret_cast<float4*>(dst) = v;
      } else {
        const int k = v0 ? 0 : 1;
        v2f y;
        y.x = yr[k];
        y.y = yi[k];
        reinterpret_cast<v2f*>(dst)[k] = y;
      }
    } else {
      const unsigned wA = iq_pack<F>(iq_store_code<F>(yr[0], a.inv_scale), iq_store_code<F>(yi[0], a.inv_scale));
      const unsigned wB = iq_pack<F>(iq_store_code<F>(yr[1], a.inv_scale), iq_store_code<F>(yi[1], a.inv_scale));
      if constexpr (SB == 4) {
        if (v0 && v1) {
          uint2 v;
          v.x = wA, v.y = wB;
          *reinterpret_cast<uint2*>(dst) = v;
        } else {
          reinterpret_cast<unsigned*>(dst)[v0 ? 0 : 1] = v0 ? wA : wB;
        }
      } else {
        if (v0 && v1)
          *reinterpret_cast<unsigned*>(dst) = wA | (wB << 16);
        else
          reinterpret_cast<unsigned short*>(dst)[v0 ? 0 : 1] = (unsigned short)(v0 ? wA : wB);
      }
    }
  }
}

// Both entries: `format` is kIqCf32 for lora_impair_batch, else the raw entry's, checked here in
// its place among the rules
int64_t impair(const float* in, int64_t rows, int64_t row_len, int64_t in_stride, int64_t first_sample,
               int64_t first_row, uint64_t seed, const float* gain, const int32_t* fcw, const int32_t* phase,
               const float* sigma, void* out, bool raw, int format, float inv_scale, int64_t out_stride, int device,
               void* stream) {
  if (rows < 0 || row_len < 0 || in_stride < 0 || out_stride < 0 || first_sample < 0 || first_row < 0)
    return set_last_error(LORA_EINVAL, "negative rows / row_len / in_stride / out_stride / first_sample / first_row");
  if (row_len >= (int64_t(1) << 31)) return set_last_error(LORA_EINVAL, "row_len must be < 2^31");
  if (rows > 1 && in && in_stride < row_len) return set_last_error(LORA_EINVAL, "in_stride smaller than row_len");
  if (rows > 1 && out_stride < row_len) return set_last_error(LORA_EINVAL, "out_stride smaller than row_len");
  if (in && static_cast<const void*>(in) == out && in_stride != out_stride)
    return set_last_error(LORA_EINVAL, "out == in needs in_stride == out_stride");
  if (reinterpret_cast<uintptr_t>(in) % sizeof(cf)) return set_last_error(LORA_EINVAL, "in is not aligned to one sample");
  // (a format that is none of the three has the smallest sample here and is refused next)
  if (reinterpret_cast<uintptr_t>(out) % (uintptr_t)iq_sample_bytes(format))
    return set_last_error(LORA_EINVAL, "out is not aligned to one sample");
  if (raw && format != LORA_IQ_CS16 && format != LORA_IQ_CS8 && format != LORA_IQ_CU8)
    return set_last_error(LORA_EINVAL, "format must be LORA_IQ_CS16, LORA_IQ_CS8 or LORA_IQ_CU8");
  ImpairArgs a{};
  a.gpr = (row_len + kTile - 1) / kTile;
  if (const char* bad = grid_error(rows, a.gpr)) return set_last_error(LORA_EINVAL, bad);
  if (rows == 0 || row_len == 0) return row_len;
  if (!out) return set_last_error(LORA_EINVAL, "null out");
  if (!in && !sigma) return set_last_error(LORA_EINVAL, "noise-only rows (in == NULL) need sigma");
  if (!gain && !fcw && !phase && !sigma)
    return set_last_error(LORA_EINVAL, "nothing to do: gain, fcw, phase and sigma are all NULL");
  a.in = reinterpret_cast<const cf*>(in);
  a.out = out;
  a.gain = gain;
  a.fcw = fcw;
  a.phase = phase;
  a.sigma = sigma;
  a.in_stride = in_stride;
  a.out_stride = out_stride;
  a.row_len = row_len;
  a.first_sample = (uint64_t)first_sample;
  a.first_row = (uint64_t)first_row;
  a.key0 = (uint32_t)seed;
  a.key1 = (uint32_t)(seed >> 32);
  a.inv_scale = inv_scale;
  void (*const kernel)(ImpairArgs) = format == LORA_IQ_CS16  ? k_impair<LORA_IQ_CS16>
                                     : format == LORA_IQ_CS8 ? k_impair<LORA_IQ_CS8>
                                     : format == LORA_IQ_CU8 ? k_impair<LORA_IQ_CU8>
                                                             : k_impair<kIqCf32>;
  return launch_bank(kernel, "k_impair", a, rows * a.gpr, kThreads, 0, device, stream, row_len);
}

}  // namespace
}  // namespace lora

extern "C" {

int64_t lora_impair_batch(const float* in, int64_t rows, int64_t row_len, int64_t in_stride, int64_t first_sample,
                          int64_t first_row, uint64_t seed, const float* gain, const int32_t* fcw,
                          const int32_t* phase, const float* sigma, float* out, int64_t out_stride, int device,
                          void* stream) {
  return lora::impair(in, rows, row_len, in_stride, first_sample, first_row, seed, gain, fcw, phase, sigma, out, false,
                      lora::kIqCf32, 0.0f, out_stride, device, stream);
}

int64_t lora_impair_raw_batch(const float* in, int64_t rows, int64_t row_len, int64_t in_stride, int64_t first_sample,
                              int64_t first_row, uint64_t seed, const float* gain, const int32_t* fcw,
                              const int32_t* phase, const float* sigma, void* out, int format, float inv_scale,
                              int64_t out_stride, int device, void* stream) {
  return lora::impair(in, rows, row_len, in_stride, first_sample, first_row, seed, gain, fcw, phase, sigma, out, true,
                      format, inv_scale, out_stride, device, stream);
}

}  // extern "C"
