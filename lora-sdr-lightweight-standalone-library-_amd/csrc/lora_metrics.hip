// lora_metrics.hip — per-symbol detector metrics (lora_demod_metrics_batch).
//
// For every whole symbol of every frame the four values LoRaDetector<float>::detect returns
// (LoRaDetector.hpp:39-74): the argmax bin, `power` (the peak in dB), `powerAvg` (everything
// but the peak, in dB) and `fIndex` (the fractional-bin offset from the two wrap-around
// neighbours).  The FFT input is the one the reference feeds for that symbol in the plan's
// mode (LoRaDemod.cpp:137-164, phy.cpp:197-227, or the bare detector of LORA_MODE_RAW), built
// from the caller's per-frame cfo / time_offset / max_amp arrays - the values
// lora_demod_batch wrote for the same frames - so no workspace is needed.
//
// The arithmetic is always the exact one (glibc-faithful sincosf / log10f / hypotf, the
// kissfft-faithful fft_lds, no contraction), whatever precision and pipeline the plan runs
// its symbols with: the outputs are defined on the exact spectrum.
//
// `total` in detect() is a double sum of the fp32 |X|^2 in bin order 0..N-1.  On a clean
// frame total - maxValue cancels almost completely, so any other summation order gives a
// different powerAvg: one lane per symbol adds that symbol's N values in order (DESIGN.md,
// "The ordered sum of the detector metrics").
#include <hip/hip_runtime.h>

#include <limits.h>

#include <string>

#include "../../include/lora_mi355x.h"
#include "lora_device.h"
#include "lora_internal.h"

#pragma clang fp contract(off)

namespace lora {
namespace {

constexpr int kThreads = 256;

// Window base of symbol s with the t_off rule (LoRaDemod.cpp:142-149, phy.cpp:205-212):
// lora_demod_fast.hip's sym_base, without the dechirp-table phase (the table index is taken
// from the sample's position in the frame here, so any t_off is covered).
__device__ __forceinline__ int64_t sym_base(int s, int step, int64_t frame_len, int t_off) {
  int64_t base = (int64_t)s * step;
  if (t_off > 0) {
    if (base + t_off + step <= frame_len) base += t_off;
  } else if (t_off < 0) {
    const int64_t off = -(int64_t)t_off;
    if (off <= base) base -= off;
  }
  return base;
}

// static_cast<int>(std::round(x)) (LoRaDemod.cpp:137, phy.cpp:197) for every float: values
// beyond int saturate and NaN gives 0, so whatever the caller's array holds, sym_base's
// guards keep the window inside the frame.
__device__ __forceinline__ int round_to_int(float x) {
  const float r = roundf(x);
  if (!(r == r)) return 0;
  if (r >= 2147483648.0f) return INT_MAX;
  if (r <= -2147483648.0f) return INT_MIN;
  return (int)r;
}

// One workgroup: G consecutive symbols of the batch (work item w = frame * total + symbol).
//   A [G][N]  the windows in kissfft's leaf order, then their spectra in natural order
//   M [N][G]  |X|^2, bin-major: the G scanning lanes read consecutive words
//   K [G]     argmax keys
__global__ void __launch_bounds__(kThreads)
k_detect_metrics(KArgs a, const float* __restrict__ cfo, const float* __restrict__ toff,
                 const float* __restrict__ max_amp, lora_symbol_metrics o, int64_t work) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int sf = a.sf, N = a.N, G = metrics_group(sf);
  cf* A = reinterpret_cast<cf*>(smem);
  float* M = reinterpret_cast<float*>(A + (size_t)G * N);
  unsigned long long* K = reinterpret_cast<unsigned long long*>(M + (size_t)G * N);
  const int tid = threadIdx.x;
  const int64_t w0 = (int64_t)blockIdx.x * G;
  // w -> (frame, symbol): one 64-bit division per workgroup, a 32-bit one per point
  const int64_t f0 = w0 / a.total;
  const uint32_t r0 = (uint32_t)(w0 - f0 * a.total);
  const uint32_t utotal = (uint32_t)a.total;
  const bool legacy = a.mode == LORA_MODE_LEGACY, api = a.mode == LORA_MODE_API;

  if (tid < G) K[tid] = 0;
  // G * N is a multiple of the 256 threads (4096, or 64 N with N >= 4)
  for (int b = tid; b < G * N; b += kThreads) {
    const int sym = b >> sf, i = b & (N - 1);
    cf v{0.0f, 0.0f};
    if (w0 + sym < work) {
      const uint32_t loc = r0 + (uint32_t)sym;
      const uint32_t q = loc / utotal;
      const int64_t f = f0 + q;
      const int s = (int)(loc - q * utotal);
      int t_off = 0;
      float rate = 0.0f;
      if (legacy || api) {
        t_off = round_to_int(toff[f]);
        rate = -2.0f * PI_F * cfo[f] / (float)N;
      }
      const uint32_t j = (uint32_t)sym_base(s, a.step, a.frame_len, t_off) + (uint32_t)i * (uint32_t)a.osr;
      v = a.iq[f * a.frame_stride + j];
      if (api) {
        v = cmul(v, a.down1[i]);  // phy.cpp:221
      } else {
        if (a.dechirp) v = cmul(v, a.down[j % (uint32_t)a.step]);  // e2e_chain_test.cpp:88-93
        if (legacy) {  // LoRaDemod.cpp:68-77
          const float m = max_amp[f];
          if (m > 1.0f) v = cscale(v, 1.0f / m);
        }
      }
      if (legacy || api) {  // LoRaDemod.cpp:151-158, phy.cpp:214-221
        const float start = rate * ((float)((uint32_t)s * (uint32_t)N) + (float)t_off / (float)a.osr);
        const float ph = start + rate * (float)i;
        float sn, cs;
        lm_sincosf(ph, &sn, &cs);
        v = cmul(v, cf{cs, sn});
      }
      if (a.hann) v = cscale(v, a.win[i]);
    }
    A[sym * N + a.rev[i]] = v;
  }
  __syncthreads();
  fft_lds(A, sf, G, a.tw, tid, kThreads);

  // |X|^2 of every bin and the lowest-index argmax (LoRaDetector.hpp:46-58).  A wave's 64
  // consecutive points belong to one symbol (N >= 64) or to 64 / N whole ones.
  const int T = N < 64 ? N : 64;
  for (int b = tid; b < G * N; b += kThreads) {
    const int sym = b >> sf, i = b & (N - 1);
    const cf v = A[b];
    M[i * G + sym] = v.re * v.re + v.im * v.im;
    const uint64_t k = group_max(argmax_key(v, (uint32_t)i), T);
    if ((tid & (T - 1)) == 0) atomicMax(&K[sym], (unsigned long long)k);
  }
  __syncthreads();

  if (tid >= G || w0 + tid >= work) return;
  double total = 0.0;  // LoRaDetector.hpp:45,52: in bin order
#pragma unroll 8
  for (int i = 0; i < N; ++i) total += (double)M[i * G + tid];
  const uint64_t key = K[tid];
  const uint32_t idx = key_index(key);
  const float maxv = key_value(key);
  const cf* X = A + tid * N;
  float power, findex;
  detect_tail(maxv, X[idx > 0 ? idx - 1 : N - 1], X[idx < (uint32_t)N - 1 ? idx + 1 : 0], a.power_scale, &power,
              &findex);
  const float noise = sqrtf((float)(total - (double)maxv));        // :60
  const float power_avg = 20.0f * lm_log10f(noise) - a.power_scale;  // :63
  const uint32_t loc = r0 + (uint32_t)tid;
  const uint32_t q = loc / utotal;
  const int64_t at = (f0 + q) * o.stride + (loc - q * utotal);
  if (o.power) o.power[at] = power;
  if (o.power_avg) o.power_avg[at] = power_avg;
  if (o.f_index) o.f_index[at] = findex;
  if (o.index) o.index[at] = (uint16_t)idx;
}

}  // namespace

// Enqueue k_detect_metrics for `frames` frames of a.total symbols each on `st`.
int launch_detect_metrics(const KArgs& a, const float* cfo, const float* toff, const float* max_amp,
                          const lora_symbol_metrics& o, int64_t frames, hipStream_t st) {
  const int G = metrics_group(a.sf);
  const int64_t work = frames * a.total;
  const int64_t grid = (work + G - 1) / G;
  if (grid >= (int64_t(1) << 31)) return set_last_error(LORA_EINVAL, "batch too large");
  const size_t lds = (size_t)G * a.N * (sizeof(cf) + sizeof(float)) + (size_t)G * sizeof(unsigned long long);
  hipLaunchKernelGGL(k_detect_metrics, dim3((unsigned)grid), dim3(kThreads), lds, st, a, cfo, toff, max_amp, o, work);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_last_error(LORA_EIO, std::string("k_detect_metrics: ") + hipGetErrorString(e));
  return LORA_OK;
}

}  // namespace lora
