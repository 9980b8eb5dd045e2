// lora_gather.hip — cut frames out of a stream of samples: lora_gather_frames_batch
// (include/lora_mi355x.h).  One kernel, k_gather_frames: slot s of the output holds the len[s]
// samples of the flat stream from sample at[s] on, then zeros up to `cut` samples.
//
// This is the stage that moves the stream's bytes between the frame finder and the
// demodulator.  A lane moves two neighbouring samples (16 bytes), neighbouring lanes
// neighbouring pairs, kPairs of them per lane 256 pairs apart: every access of a wave is one
// contiguous KiB.  The output's rows are 16-byte aligned and written with 16-byte stores.  A
// frame starts at any sample, so its source is only 8-byte aligned: a slot whose source is
// 16-byte aligned reads 16 bytes per lane, any other reads the pair as two 8-byte loads (the
// wave still touches the same contiguous KiB).  The choice is uniform over a workgroup, which
// works on one slot.  Nothing at or beyond at + len, or beyond the stream's end, is read.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/lora_mi355x.h"
#include "lora_internal.h"

namespace {

constexpr int kBlock = 256;
constexpr int kPairs = 4;                       // pairs of samples per lane
constexpr int kChunk = 2 * kPairs * kBlock;     // samples per workgroup

struct GatherArgs {
  const float2* flat;
  int64_t total;
  const int64_t* at;
  const int64_t* len;
  int64_t cut, out_stride;
  float2* out;
  int chunks;  // workgroups per slot
};

__global__ void __launch_bounds__(kBlock) k_gather_frames(GatherArgs a) {
  const int64_t slot = blockIdx.x / (unsigned)a.chunks;
  const int chunk = (int)(blockIdx.x - slot * a.chunks);
  const int64_t at = a.at[slot];
  int64_t n = 0;  // samples to copy
  if (at >= 0 && at < a.total) {
    const int64_t room = a.total - at < a.cut ? a.total - at : a.cut;
    n = a.len[slot];
    n = n < 0 ? 0 : (n < room ? n : room);
  }
  const float2* src = a.flat + (n > 0 ? at : 0);
  float2* dst = a.out + slot * a.out_stride;
  const bool aligned = (reinterpret_cast<uintptr_t>(src) & 15) == 0;
#pragma unroll
  for (int u = 0; u < kPairs; ++u) {
    const int64_t t = (int64_t)chunk * kChunk + 2 * (u * kBlock + (int)threadIdx.x);
    if (t >= a.cut) continue;
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (t + 1 < n) {
      if (aligned) {
        v = *reinterpret_cast<const float4*>(src + t);
      } else {
        const float2 x = src[t], y = src[t + 1];
        v = make_float4(x.x, x.y, y.x, y.y);
      }
    } else if (t < n) {
      const float2 x = src[t];
      v.x = x.x;
      v.y = x.y;
    }
    if (t + 1 < a.cut)
      *reinterpret_cast<float4*>(dst + t) = v;
    else
      dst[t] = make_float2(v.x, v.y);  // the last sample of an odd cut
  }
}

}  // namespace

using lora::set_last_error;

int64_t lora_gather_frames_batch(const float* flat, int64_t total, const int64_t* at, const int64_t* len,
                                 int64_t slots, int64_t cut, float* out, int64_t out_stride, int device,
                                 void* stream) {
  if (total < 0 || slots < 0 || cut < 0) return set_last_error(LORA_EINVAL, "bad total / slots / cut");
  if (out_stride < cut) return set_last_error(LORA_EINVAL, "out_stride smaller than cut");
  if (slots == 0 || cut == 0) return cut;
  if (!at || !len || !out || (total > 0 && !flat)) return set_last_error(LORA_EINVAL, "null buffer");
  if ((reinterpret_cast<uintptr_t>(flat) & 7) || (reinterpret_cast<uintptr_t>(out) & 15) ||
      (slots > 1 && (out_stride & 1)))
    return set_last_error(LORA_EINVAL, "flat must be 8-byte aligned, out and its rows 16-byte aligned");
  const int64_t chunks = (cut + kChunk - 1) / kChunk;
  if (chunks >= (int64_t(1) << 31) / slots) return set_last_error(LORA_EINVAL, "batch too large");
  GatherArgs a;
  a.flat = reinterpret_cast<const float2*>(flat);
  a.total = total;
  a.at = at;
  a.len = len;
  a.cut = cut;
  a.out_stride = out_stride;
  a.out = reinterpret_cast<float2*>(out);
  a.chunks = (int)chunks;
  lora::DeviceGuard guard(device);
  if (guard.err != hipSuccess) return lora::hip_error("gather device", guard.err);
  hipLaunchKernelGGL(k_gather_frames, dim3((unsigned)(slots * chunks)), dim3(kBlock), 0,
                     static_cast<hipStream_t>(stream), a);
  const hipError_t e = hipGetLastError();
  return e != hipSuccess ? lora::hip_error("gather launch", e) : cut;
}
