// lora_iq_format.h — the sample formats the down-converter banks read (include/lora_mi355x.h,
// LORA_IQ_*; 0 is complex64 here) and the one loop of either bank that knows them: the load in
// front of `mix` (csrc/lora_channelize.hip, csrc/lora_resample.hip); and the store side of the
// same formats, fp32 to a stored code, for the synthesis bank (csrc/lora_synth.hip).
//
// A stored integer component v becomes x = ((float)v - bias) * scale, fp32, one rounding per
// operation, no contraction; bias is 127.5f for cu8 and nothing for the signed formats.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lora_mi355x.h"
#include "lora_device.h"

#pragma clang fp contract(off)

namespace lora {

constexpr int kIqCf32 = 0;  // complex64, the float entries' format

__host__ __device__ constexpr int iq_sample_bytes(int format) {
  return format == kIqCf32 ? 8 : format == LORA_IQ_CS16 ? 4 : 2;
}

// One stored sample of an integer format, I in the low half of `w` and Q above it
// (little-endian), to fp32 by the definition above
template <int F>
__device__ __forceinline__ void iq_convert(unsigned w, float scale, float& xr, float& xi) {
  if constexpr (F == LORA_IQ_CS16) {
    xr = (float)(short)(w & 0xffffu) * scale;
    xi = (float)(short)(w >> 16) * scale;
  } else if constexpr (F == LORA_IQ_CS8) {
    xr = (float)(signed char)(w & 0xffu) * scale;
    xi = (float)(signed char)((w >> 8) & 0xffu) * scale;
  } else {
    static_assert(F == LORA_IQ_CU8, "unknown sample format");
    xr = ((float)(w & 0xffu) - 127.5f) * scale;
    xi = ((float)((w >> 8) & 0xffu) - 127.5f) * scale;
  }
}

// mix(s, xr, xi) for every sample s in 0 .. cnt-1 of the row part that begins `first` samples
// after `iq`.  A lane takes two samples per round with one load of a pair's size - 16 bytes of
// complex64, 8 of cs16, 4 of an 8-bit format - on that size's grid of the address space: pair q
// holds samples 2q - mis and 2q + 1 - mis; a pair that hangs over either end is loaded singly.
// So consecutive lanes read consecutive addresses whatever the format, every lane mixes its two
// samples as the complex64 path's lanes do, and `iq` need only be aligned to one sample.
// (Measured, profiles/channel/raw_time.json: 16-byte loads of an integer format, each shared
// by the 2 or 4 neighbouring lanes that split its samples, took 1.15 - 1.18 times this form's
// time in the rational bank and 1.00 - 1.04 times it in the integer one.)
template <int F, class Mix>
__device__ __forceinline__ void load_samples(const void* iq, int64_t first, int cnt, float scale, int tid,
                                             int threads, Mix&& mix) {
  constexpr int SB = iq_sample_bytes(F);
  const unsigned char* x = static_cast<const unsigned char*>(iq) + first * SB;
  auto single = [&](int s) {
    if constexpr (F == kIqCf32) {
      const cf v = reinterpret_cast<const cf*>(x)[s];
      mix(s, v.re, v.im);
    } else {
      float xr, xi;
      if constexpr (SB == 4)
        iq_convert<F>(reinterpret_cast<const unsigned*>(x)[s], scale, xr, xi);
      else
        iq_convert<F>(reinterpret_cast<const unsigned short*>(x)[s], scale, xr, xi);
      mix(s, xr, xi);
    }
  };
  const int mis = (int)((reinterpret_cast<uintptr_t>(x) / SB) & 1);
  const int pairs = (cnt + mis + 1) / 2;
  for (int q = tid; q < pairs; q += threads) {
    const int s0 = 2 * q - mis;
    if (s0 >= 0 && s0 + 2 <= cnt) {
      const unsigned char* p = x + (int64_t)s0 * SB;  // on the pair's grid
      if constexpr (F == kIqCf32) {
        const float4 v = *reinterpret_cast<const float4*>(p);
        mix(s0, v.x, v.y);
        mix(s0 + 1, v.z, v.w);
      } else {
        unsigned w0, w1;
        if constexpr (SB == 4) {  // a sample to a word
          const uint2 v = *reinterpret_cast<const uint2*>(p);
          w0 = v.x;
          w1 = v.y;
        } else {  // two samples to a word
          const unsigned w = *reinterpret_cast<const unsigned*>(p);
          w0 = w & 0xffffu;
          w1 = w >> 16;
        }
        float xr, xi;
        iq_convert<F>(w0, scale, xr, xi);
        mix(s0, xr, xi);
        iq_convert<F>(w1, scale, xr, xi);
        mix(s0 + 1, xr, xi);
      }
    } else {
      // (This loop's bounds are written as they were measured, each end tested for each sample
      // though one test each would do.  With the previous loop's own expressions here the
      // complex64 kernels came out scheduled otherwise and took 1.015 - 1.027 times their
      // previous time; in this form 0.978 - 0.993 times: float_loop_forms in the record.)
      if (s0 >= 0 && s0 < cnt) single(s0);
      if (s0 + 1 >= 0 && s0 + 1 < cnt) single(s0 + 1);
    }
  }
}

// The store side (csrc/lora_synth.hip): an fp32 component y to the stored code of an integer
// format, v = y * inv_scale (one product), for cu8 v = v + 127.5f (one sum), then
// clamp(rintf(v), lo, hi) with ties to even; a NaN v stores the format's zero (0, or 128 for cu8)
template <int F>
__device__ __forceinline__ int iq_store_code(float y, float inv_scale) {
  static_assert(F == LORA_IQ_CS16 || F == LORA_IQ_CS8 || F == LORA_IQ_CU8, "unknown sample format");
  constexpr float lo = F == LORA_IQ_CS16 ? -32768.0f : F == LORA_IQ_CS8 ? -128.0f : 0.0f;
  constexpr float hi = F == LORA_IQ_CS16 ? 32767.0f : F == LORA_IQ_CS8 ? 127.0f : 255.0f;
  float v = y * inv_scale;
  if constexpr (F == LORA_IQ_CU8) v = v + 127.5f;
  if (v != v) return F == LORA_IQ_CU8 ? 128 : 0;
  return (int)fminf(fmaxf(rintf(v), lo), hi);
}

// The codes of I and Q as one stored sample, I in the low half (little-endian): 32 bits of cs16,
// 16 of an 8-bit format
template <int F>
__device__ __forceinline__ unsigned iq_pack(int ci, int cq) {
  if constexpr (F == LORA_IQ_CS16)
    return ((unsigned)ci & 0xffffu) | ((unsigned)cq << 16);
  else
    return ((unsigned)ci & 0xffu) | (((unsigned)cq & 0xffu) << 8);
}

// The raw entries' checks that the float entries do not have (host): the format is one of
// LORA_IQ_*, and iq is aligned to one sample
inline const char* raw_format_error(const void* iq, int format) {
  if (format != LORA_IQ_CS16 && format != LORA_IQ_CS8 && format != LORA_IQ_CU8)
    return "format must be LORA_IQ_CS16, LORA_IQ_CS8 or LORA_IQ_CU8";
  if (reinterpret_cast<uintptr_t>(iq) % (uintptr_t)iq_sample_bytes(format))
    return "iq is not aligned to one sample";
  return nullptr;
}

}  // namespace lora
