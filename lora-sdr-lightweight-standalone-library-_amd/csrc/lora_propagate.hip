// lora_propagate.hip — the propagation stage (lora_propagate_batch): what stands between the
// synthesis bank and the impairment stage.  Rows of complex64 in, rows of complex64 out, each
// output the sum of up to eight paths, every path the recording read at a fractional position
// (an integer-word delay plus a sample-clock offset that slides it) through a table of 256
// fractional-delay filters and weighted by a complex gain; then a carrier whose frequency may
// drift (a 64-bit phase accumulator with a quadratic term).  The arithmetic is the header's,
// operation for operation: int64 positions, fp32 sums with one rounding each and no contraction,
// glibc's sincosf to the bit (csrc/lora_libm.h).  The definition is this library's own
// (tests/propagate_checker.py restates it in numpy and the GPU tests compare bits).
//
// A sample's value depends on (n, its row's parameters, the recording) alone, so nothing below -
// the tile, the staging, which lane holds a sample - can show in the bits.
//
// A workgroup of 256 lanes owns kTile = 1024 consecutive slots of one row, the slots laid on the
// grid of two stored output samples (slot 0 of a row whose `out` is 8 bytes off that grid is the
// sample in front of the row and is not written), so that every lane's two pairs of outputs leave
// with one 16-byte store each; the one sample that hangs over an end of the row goes singly.
// The paths are staged in turn, not together: each path's positions over the tile are a run of
// at most kTile + taps + 1 consecutive recording samples (|sfo| <= 2^20 moves a path by less than
// a quarter of a sample over a tile), loaded once into LDS with 16-byte loads on the input's own
// 16-byte grid and zero-filled outside the `in` window; paths whose delays lie close would share
// most of a staging, but a shared window would have to be sized for the farthest pair and the
// load is not what bounds the kernel.  The table's phase moves by at most
// 64 rows over a tile, so the rows a tile can touch (65 at most, wrapping modulo 256) are staged
// beside the samples at a pitch of 33 floats: a wave's lanes read one or two neighbouring rows,
// the same address (a broadcast) or different banks.  An output's taps then run out of LDS: one
// 8-byte sample and one 4-byte coefficient per tap.  The four angles of a lane's outputs go
// through one interleaved four-way sincos (lm_sincosf_fast_k), as the impairment stage's do.
// The row's parameters are uniform over the workgroup: scalar loads.
//
// delay and sfo live on the device, so the kernel cannot refuse them: a value beyond the header's
// limits gives samples that are not the definition's, but every LDS index is clamped into what
// was staged and nothing outside `in`'s window and `out`'s rows is touched.
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
constexpr int kMaxTaps = 32, kMaxPaths = 8;
constexpr int kStage = kTile + kMaxTaps + 8;  // tile + taps + one step of q + one for the 16-byte grid, rounded up
constexpr int kPhases = 65;                   // table rows a tile can touch: 1023 * 2^20 / 2^24 < 64 steps
constexpr int kPitch = kMaxTaps + 1;
constexpr float kWordToRad = 0x1.921fb6p-30f;  // fp32 pi * 2^-31: a signed 32-bit word to (-pi, pi]

struct PropArgs {
  const cf* in;
  cf* out;
  const int64_t* delay;
  const float* gain;
  const int64_t* sfo;
  const float* table;
  const int64_t* fcw;
  const int64_t* rate;
  const int32_t* phase;
  int64_t in_len, in_stride, in_first, row_len, out_stride, first_sample, gpr;
  int paths, taps;
};

__device__ __forceinline__ int clampi(int64_t v, int lo, int hi) {
  return v < lo ? lo : v > hi ? hi : (int)v;
}

__global__ void __launch_bounds__(kThreads) k_propagate(PropArgs a) {
  __shared__ __attribute__((aligned(16))) v2f S[kStage];
  __shared__ float Tb[kPhases * kPitch];

  const int tid = threadIdx.x;
  const int64_t row = (int64_t)blockIdx.x / a.gpr;
  cf* orow = a.out + row * a.out_stride;
  // the tile's first slot as an output index: even slots lie on the 16-byte grid of `out`
  const int64_t tb = ((int64_t)blockIdx.x - row * a.gpr) * kTile - (int64_t)((reinterpret_cast<uintptr_t>(orow) >> 3) & 1);
  const int64_t ts = tb < 0 ? 0 : tb;
  const int64_t te = tb + kTile < a.row_len ? tb + kTile : a.row_len;
  if (ts >= te) return;  // (the whole workgroup: the last tile of a row that needs no slot of it)

  const int T = a.taps, P = a.paths, h = T / 2 - 1;
  const int64_t sfo = a.sfo ? a.sfo[row] : 0;
  const int64_t nA = a.first_sample + ts, nB = a.first_sample + te - 1;
  const cf* irow = a.in + row * a.in_stride;

  float yr[4] = {0.0f, 0.0f, 0.0f, 0.0f}, yi[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int p = 0; p < P; ++p) {
    const int64_t d = a.delay[row * P + p];
    const float gr = a.gain[(row * P + p) * 2], gi = a.gain[(row * P + p) * 2 + 1];
    // n + q never decreases with n, so the tile's first and last outputs bound what it reads
    const int64_t mA = -(d + sfo * nA), mB = -(d + sfo * nB);
    const int64_t jlo = nA + (mA >> 32) - h;
    const int64_t jhi = nB + (mB >> 32) - h + (T - 1);
    int64_t e0 = jlo - a.in_first;  // the first staged sample as an element of the row of `in`
    e0 -= (int64_t)(((reinterpret_cast<uintptr_t>(irow) >> 3) + (uint64_t)e0) & 1);  // onto the 16-byte grid
    const int64_t base = e0 + a.in_first;
    const int cnt = clampi(jhi - base + 1, 0, kStage);
    const int64_t glo = (mA < mB ? mA : mB) >> 24;
    const int nph = clampi(((mA < mB ? mB : mA) >> 24) - glo + 1, 1, kPhases);

    __syncthreads();  // the previous path's taps have been read
    for (int i = tid; 2 * i < cnt; i += kThreads) {
      const int64_t e = e0 + 2 * i;
      float4 v = {0.0f, 0.0f, 0.0f, 0.0f};
      if (e >= 0 && e + 1 < a.in_len) {
        v = *reinterpret_cast<const float4*>(irow + e);
      } else {
        if (e >= 0 && e < a.in_len) {
          const cf u = irow[e];
          v.x = u.re, v.y = u.im;
        }
        if (e + 1 >= 0 && e + 1 < a.in_len) {
          const cf u = irow[e + 1];
          v.z = u.re, v.w = u.im;
        }
      }
      *reinterpret_cast<float4*>(&S[2 * i]) = v;
    }
    for (int r = tid >> 5, t = tid & 31; r < nph; r += kThreads / 32)
      if (t < T) Tb[r * kPitch + t] = a.table[(int)((glo + r) & 255) * T + t];
    __syncthreads();

#pragma unroll
    for (int o = 0; o < 4; ++o) {
      // (a slot outside the row computes on clamped indices and is not stored)
      const int64_t n = a.first_sample + tb + 2 * (tid + kThreads * (o >> 1)) + (o & 1);
      const int64_t m = -(d + sfo * n);
      const v2f* sp = S + clampi(n + (m >> 32) - h - base, 0, kStage - T);
      const float* tp = Tb + clampi((m >> 24) - glo, 0, kPhases - 1) * kPitch;
      float sr = 0.0f, si = 0.0f;
#pragma unroll 2
      for (int t = 0; t < T; ++t) {
        const float w = tp[t];
        const v2f x = sp[t];
        sr = sr + w * x.x;
        si = si + w * x.y;
      }
      const float cr = gr * sr - gi * si;
      const float ci = gr * si + gi * sr;
      yr[o] = yr[o] + cr;
      yi[o] = yi[o] + ci;
    }
  }

  if (a.fcw != nullptr || a.rate != nullptr || a.phase != nullptr) {
    const uint64_t fcw = a.fcw ? (uint64_t)a.fcw[row] : 0u;
    const uint64_t rate = a.rate ? (uint64_t)a.rate[row] : 0u;
    const uint64_t ph0 = a.phase ? (uint64_t)(uint32_t)a.phase[row] << 32 : 0u;
    float ang[4], sn[4], cs[4];
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      const uint64_t n = (uint64_t)(a.first_sample + tb + 2 * (tid + kThreads * (o >> 1)) + (o & 1));
      const uint64_t tri = (n & 1) ? n * ((n - 1) >> 1) : (n >> 1) * (n - 1);
      const uint64_t W = ph0 + fcw * n + rate * tri;
      ang[o] = (float)(int32_t)(uint32_t)(W >> 32) * kWordToRad;
    }
    lm_sincosf_fast_k<4>(ang, sn, cs);
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      const float xr = yr[o], xi = yi[o];
      yr[o] = xr * cs[o] - xi * sn[o];
      yi[o] = xr * sn[o] + xi * cs[o];
    }
  }

#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int64_t s0 = tb + 2 * (tid + kThreads * r);  // on the grid of two stored samples
    const bool v0 = s0 >= ts && s0 < te, v1 = s0 + 1 < te;  // (s0 + 1 >= ts always)
    if (v0 && v1) {
      float4 v;
      v.x = yr[2 * r], v.y = yi[2 * r], v.z = yr[2 * r + 1], v.w = yi[2 * r + 1];
      *reinterpret_cast<float4*>(orow + s0) = v;
    } else if (v0 || v1) {
      const int k = v0 ? 0 : 1;
      v2f y;
      y.x = yr[2 * r + k];
      y.y = yi[2 * r + k];
      *reinterpret_cast<v2f*>(orow + s0 + k) = y;
    }
  }
}

// the bytes rows of `len` samples `stride` apart span, saturated: 0 when there is nothing
uint64_t span_bytes(int64_t rows, int64_t len, int64_t stride) {
  if (rows <= 0 || len <= 0) return 0;
  const uint64_t cap = uint64_t(1) << 60;
  if (stride > 0 && (uint64_t)(rows - 1) > cap / (uint64_t)stride) return cap * sizeof(cf);
  const uint64_t n = (uint64_t)(rows - 1) * (uint64_t)stride + (uint64_t)len;
  return (n > cap ? cap : n) * sizeof(cf);
}

}  // namespace
}  // namespace lora

extern "C" {

int64_t lora_propagate_batch(const float* in, int64_t rows, int64_t in_len, int64_t in_stride, int64_t in_first,
                             int64_t row_len, int64_t first_sample, int64_t paths, const int64_t* delay,
                             const float* gain, const int64_t* sfo, const float* table, int64_t taps,
                             const int64_t* fcw, const int64_t* rate, const int32_t* phase, float* out,
                             int64_t out_stride, int device, void* stream) {
  using namespace lora;
  constexpr int64_t kEnd = int64_t(1) << 40;
  if (rows < 0 || in_len < 0 || in_stride < 0 || in_first < 0 || row_len < 0 || first_sample < 0 || out_stride < 0)
    return set_last_error(LORA_EINVAL,
                          "negative rows / in_len / in_stride / in_first / row_len / first_sample / out_stride");
  if (row_len >= (int64_t(1) << 31)) return set_last_error(LORA_EINVAL, "row_len must be < 2^31");
  if (first_sample > kEnd - row_len || in_first > 2 * kEnd)
    return set_last_error(LORA_EINVAL, "first_sample + row_len must be <= 2^40 and in_first <= 2^41");
  if (rows > 1 && in_stride < in_len) return set_last_error(LORA_EINVAL, "in_stride smaller than in_len");
  if (rows > 1 && out_stride < row_len) return set_last_error(LORA_EINVAL, "out_stride smaller than row_len");
  if (reinterpret_cast<uintptr_t>(in) % sizeof(cf)) return set_last_error(LORA_EINVAL, "in is not aligned to one sample");
  if (reinterpret_cast<uintptr_t>(out) % sizeof(cf))
    return set_last_error(LORA_EINVAL, "out is not aligned to one sample");
  if (in && out) {
    const uint64_t ib = span_bytes(rows, in_len, in_stride), ob = span_bytes(rows, row_len, out_stride);
    const uintptr_t i0 = reinterpret_cast<uintptr_t>(in), o0 = reinterpret_cast<uintptr_t>(out);
    if (ib && ob && i0 < o0 + ob && o0 < i0 + ib) return set_last_error(LORA_EINVAL, "in and out overlap");
  }
  if (paths < 1 || paths > kMaxPaths) return set_last_error(LORA_EINVAL, "paths must be in 1..8");
  if (taps < 2 || taps > kMaxTaps || (taps & 1)) return set_last_error(LORA_EINVAL, "taps must be even and in 2..32");
  if (rows == 0 || row_len == 0) return row_len;
  if (!delay || !gain || !table || !out || (!in && in_len > 0))
    return set_last_error(LORA_EINVAL, "null in / delay / gain / table / out");
  PropArgs a{};
  // (one slot more than the row: a row that starts 8 bytes off the 16-byte grid starts at slot 1)
  a.gpr = (row_len + 1 + kTile - 1) / kTile;
  if (const char* bad = grid_error(rows, a.gpr)) return set_last_error(LORA_EINVAL, bad);
  a.in = reinterpret_cast<const cf*>(in);
  a.out = reinterpret_cast<cf*>(out);
  a.delay = delay;
  a.gain = gain;
  a.sfo = sfo;
  a.table = table;
  a.fcw = fcw;
  a.rate = rate;
  a.phase = phase;
  a.in_len = in_len;
  a.in_stride = in_stride;
  a.in_first = in_first;
  a.row_len = row_len;
  a.out_stride = out_stride;
  a.first_sample = first_sample;
  a.paths = (int)paths;
  a.taps = (int)taps;
  return launch_bank(k_propagate, "k_propagate", a, rows * a.gpr, kThreads, 0, device, stream, row_len);
}

}  // extern "C"
