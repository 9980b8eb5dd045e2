// lora_metrics.hip — per-symbol detector metrics (lora_demod_metrics_batch) and soft bits
// (lora_demod_soft_bits_batch, k_soft_bits below: another reduction of the same spectra; and
// lora_demod_soft_bits_frame_batch, k_soft_bits_frame, whose chosen columns are read as the
// header symbols of a self-describing frame).
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

// The front half both kernels share: the FFT inputs of the workgroup's G symbols (work items
// w0 .. w0 + G - 1, the first one symbol r0 of frame f0), built as the reference builds them in
// a.mode, into A in kissfft's leaf order; work items beyond `work` are zero windows.
__device__ __forceinline__ void load_windows(const KArgs& a, const float* __restrict__ cfo,
                                             const float* __restrict__ toff, const float* __restrict__ max_amp,
                                             cf* A, int sf, int G, int64_t w0, int64_t f0, uint32_t r0,
                                             int64_t work, int tid) {
  const int N = 1 << sf;
  const uint32_t utotal = (uint32_t)a.total;
  const bool legacy = a.mode == LORA_MODE_LEGACY, api = a.mode == LORA_MODE_API;
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

  if (tid < G) K[tid] = 0;
  load_windows(a, cfo, toff, max_amp, A, sf, G, w0, f0, r0, work, tid);
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


// ---- soft bits ------------------------------------------------------------------------------
// max over an aligned group of T lanes (T a power of two <= 64) of a non-negative float's bits
__device__ __forceinline__ uint32_t group_umax(uint32_t v, int T) {
  for (int s = T >> 1; s > 0; s >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, s, 64));
  return v;
}
__device__ __forceinline__ uint32_t parity(uint32_t x) { return (uint32_t)__popc(x) & 1u; }

// lora_demod_soft_bits_batch: k_detect_metrics' windows and spectra (the same G symbols per
// workgroup), then per symbol and bit c the two maxima of Q[k] = |X[k]|^2 (> 0, else 0) over
// the bins whose grayToBinary16(k) has bit c set / clear.  Bit c of grayToBinary16(k) is the
// parity of k >> c.  Q >= +0 is never NaN, so the maxima are taken on the bit patterns as
// unsigned integers (exact, any order).
//   1. every thread squares its 16 points of the natural-order pass (b = tid + 256 r);
//   2. the values go back into the dead spectrum storage as 256 runs of 16 bins, a run every
//      17 words, so that thread t reads run t (bins k = 16 j + u of one symbol, j = t mod N/16)
//      without bank conflicts;
//   3. in registers, bits 0-3: the maxima over the u with parity(u >> c) set / clear, swapped
//      where parity(j) is odd; bits c >= 4: the run's maximum on the side parity(j >> (c - 4));
//   4. the 2 SF values are reduced over the symbol's lanes of a wave (N/16, at most 64) with
//      cross-lane moves, and over its waves (SF 11: 2, SF 12: 4) through R;
//   5. llr = m1 - m0 (+0 where equal), G * SF consecutive floats per workgroup and frame.
// LDS: the 32 KiB of spectra; the runs (17 KiB) and R (at most 3 KiB at SF 6) reuse them.
//
// RED (lora_demod_soft_bits_frame_batch, k_soft_bits_frame): columns red_first .. red_first +
// red_count - 1 of every frame are those of a frame's header block, whose value is
// grayToBinary16(((k + 2) >> 2) & (2^(SF-2) - 1)).  Its bit c is bit c + 2 of
// grayToBinary16((k + 2) mod N): in step 2 such a symbol's bin k is written where bin
// (k + 2) mod N goes, and in step 5 slot c takes the maxima of bit c + 2 (slots SF-2 and SF-1:
// +0).  With RED off nothing of this is compiled: that instance is k_soft_bits, unchanged in
// its source, name, arguments and outputs.
template <int SF, bool RED>
__device__ __forceinline__ void soft_bits_body(const KArgs& a, const float* __restrict__ cfo,
                                               const float* __restrict__ toff, const float* __restrict__ max_amp,
                                               float* __restrict__ llr, int64_t llr_stride, int64_t work,
                                               uint32_t red_first, uint32_t red_count) {
  constexpr int N = 1 << SF, G = metrics_group(SF);
  constexpr int kRun = 16, kPitch = kRun + 1;
  constexpr int TN = N / kRun;               // lanes per symbol
  constexpr int TL = TN < 64 ? TN : 64;      // ... of one wave
  constexpr int WN = TN / TL;                // waves per symbol
  constexpr int kRuns = G * N / kRun;        // = kThreads
  static_assert(G * N == kRun * kThreads, "one run of 16 bins per thread");
  static_assert((kRuns * kPitch + G * WN * 2 * SF) * sizeof(float) <= (size_t)G * N * sizeof(cf), "LDS reuse");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  cf* A = reinterpret_cast<cf*>(smem);
  uint32_t* Qs = reinterpret_cast<uint32_t*>(smem);
  uint32_t* R = Qs + kRuns * kPitch;  // [G][WN][SF][2]
  const int tid = threadIdx.x;
  const int64_t w0 = (int64_t)blockIdx.x * G;
  const int64_t f0 = w0 / a.total;
  const uint32_t r0 = (uint32_t)(w0 - f0 * a.total);
  const uint32_t utotal = (uint32_t)a.total;

  load_windows(a, cfo, toff, max_amp, A, SF, G, w0, f0, r0, work, tid);
  __syncthreads();
  fft_lds(A, SF, G, a.tw, tid, kThreads);

  uint32_t q[kRun];
#pragma unroll
  for (int r = 0; r < kRun; ++r) {
    const cf v = A[tid + r * kThreads];
    const float p = v.re * v.re + v.im * v.im;  // LoRaDetector.hpp:51
    q[r] = __float_as_uint(p > 0.0f ? p : 0.0f);
  }
  __syncthreads();  // every spectrum is read: its storage is free
#pragma unroll
  for (int r = 0; r < kRun; ++r) {
    int b = tid + r * kThreads;
    if constexpr (RED) {  // a header symbol: bin k goes where bin (k + 2) mod N does
      const uint32_t col = (r0 + (uint32_t)(b >> SF)) % utotal;
      if (col - red_first < red_count) b = (b & ~(N - 1)) | ((b + 2) & (N - 1));
    }
    Qs[b + (b >> 4)] = q[r];  // run b / 16, word b % 16
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < kRun; ++u) q[u] = Qs[tid * kPitch + u];

  const uint32_t j = (uint32_t)tid & (TN - 1);  // run j of symbol tid / TN
  uint32_t m[2 * SF];  // [c][0] = bit clear, [c][1] = bit set
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    uint32_t e0 = 0, e1 = 0;
#pragma unroll
    for (int u = 0; u < kRun; ++u) {
      if ((__builtin_popcount(u >> c) & 1) != 0)
        e1 = max(e1, q[u]);
      else
        e0 = max(e0, q[u]);
    }
    const bool odd = parity(j) != 0;
    m[2 * c] = odd ? e1 : e0;
    m[2 * c + 1] = odd ? e0 : e1;
  }
  const uint32_t t = max(m[0], m[1]);
#pragma unroll
  for (int c = 4; c < SF; ++c) {
    const bool set = parity(j >> (c - 4)) != 0;
    m[2 * c] = set ? 0u : t;
    m[2 * c + 1] = set ? t : 0u;
  }
#pragma unroll
  for (int i = 0; i < 2 * SF; ++i) m[i] = group_umax(m[i], TL);
  if ((tid & (TL - 1)) == 0) {
    uint32_t* dst = R + (size_t)(tid / TL) * (2 * SF);  // (sym * WN + wave of the symbol)
#pragma unroll
    for (int i = 0; i < 2 * SF; ++i) dst[i] = m[i];
  }
  __syncthreads();

  for (int e = tid; e < G * SF; e += kThreads) {
    const int s = e / SF, c = e - s * SF;
    if (w0 + s >= work) break;
    int cc = c;  // the bit whose maxima slot c takes
    if constexpr (RED) {
      if ((r0 + (uint32_t)s) % utotal - red_first < red_count) cc = c + 2;
    }
    uint32_t m0 = 0, m1 = 0;
    if (!RED || cc < SF) {
#pragma unroll
      for (int w = 0; w < WN; ++w) {
        m0 = max(m0, R[((s * WN + w) * SF + cc) * 2]);
        m1 = max(m1, R[((s * WN + w) * SF + cc) * 2 + 1]);
      }
    }
    const uint32_t loc = r0 + (uint32_t)s;
    const uint32_t fq = loc / utotal;
    const int64_t at = ((f0 + fq) * llr_stride + (loc - fq * utotal)) * SF + c;
    llr[at] = m1 == m0 ? 0.0f : __uint_as_float(m1) - __uint_as_float(m0);
  }
}

template <int SF>
__global__ void __launch_bounds__(kThreads)
k_soft_bits(KArgs a, const float* __restrict__ cfo, const float* __restrict__ toff,
            const float* __restrict__ max_amp, float* __restrict__ llr, int64_t llr_stride, int64_t work) {
  soft_bits_body<SF, false>(a, cfo, toff, max_amp, llr, llr_stride, work, 0u, 0u);
}

template <int SF>
__global__ void __launch_bounds__(kThreads)
k_soft_bits_frame(KArgs a, const float* __restrict__ cfo, const float* __restrict__ toff,
                  const float* __restrict__ max_amp, float* __restrict__ llr, int64_t llr_stride, int64_t work,
                  uint32_t red_first, uint32_t red_count) {
  static_assert(SF >= 7, "the header block carries SF - 2 >= 5 bits");
  soft_bits_body<SF, true>(a, cfo, toff, max_amp, llr, llr_stride, work, red_first, red_count);
}

template <int SF>
void launch_soft_sf(const KArgs& a, const float* cfo, const float* toff, const float* max_amp, float* llr,
                    int64_t llr_stride, int64_t work, unsigned grid, hipStream_t st) {
  constexpr size_t lds = (size_t)metrics_group(SF) * (1 << SF) * sizeof(cf);
  hipLaunchKernelGGL(k_soft_bits<SF>, dim3(grid), dim3(kThreads), lds, st, a, cfo, toff, max_amp, llr, llr_stride,
                     work);
}

template <int SF>
void launch_soft_frame_sf(const KArgs& a, const float* cfo, const float* toff, const float* max_amp, float* llr,
                          int64_t llr_stride, int64_t work, unsigned grid, hipStream_t st, uint32_t red_first,
                          uint32_t red_count) {
  constexpr size_t lds = (size_t)metrics_group(SF) * (1 << SF) * sizeof(cf);
  hipLaunchKernelGGL(k_soft_bits_frame<SF>, dim3(grid), dim3(kThreads), lds, st, a, cfo, toff, max_amp, llr,
                     llr_stride, work, red_first, red_count);
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

// Enqueue k_soft_bits for `frames` frames of a.total symbols each on `st` (a.sf in 6..12).
int launch_soft_bits(const KArgs& a, const float* cfo, const float* toff, const float* max_amp, float* llr,
                     int64_t llr_stride, int64_t frames, hipStream_t st) {
  const int G = metrics_group(a.sf);
  const int64_t work = frames * a.total;
  const int64_t grid = (work + G - 1) / G;
  if (grid >= (int64_t(1) << 31)) return set_last_error(LORA_EINVAL, "batch too large");
  const unsigned g = (unsigned)grid;
  switch (a.sf) {
    case 6: launch_soft_sf<6>(a, cfo, toff, max_amp, llr, llr_stride, work, g, st); break;
    case 7: launch_soft_sf<7>(a, cfo, toff, max_amp, llr, llr_stride, work, g, st); break;
    case 8: launch_soft_sf<8>(a, cfo, toff, max_amp, llr, llr_stride, work, g, st); break;
    case 9: launch_soft_sf<9>(a, cfo, toff, max_amp, llr, llr_stride, work, g, st); break;
    case 10: launch_soft_sf<10>(a, cfo, toff, max_amp, llr, llr_stride, work, g, st); break;
    case 11: launch_soft_sf<11>(a, cfo, toff, max_amp, llr, llr_stride, work, g, st); break;
    case 12: launch_soft_sf<12>(a, cfo, toff, max_amp, llr, llr_stride, work, g, st); break;
    default: return set_last_error(LORA_EINVAL, "soft bits need sf in 6..12");
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_last_error(LORA_EIO, std::string("k_soft_bits: ") + hipGetErrorString(e));
  return LORA_OK;
}

// Enqueue k_soft_bits_frame (a.sf in 7..12): columns red_first .. red_first + red_count - 1 of
// every frame are reduced (0 <= red_first, 0 < red_count, red_first + red_count <= a.total).
int launch_soft_bits_frame(const KArgs& a, const float* cfo, const float* toff, const float* max_amp, float* llr,
                           int64_t llr_stride, int64_t frames, int64_t red_first, int64_t red_count, hipStream_t st) {
  const int G = metrics_group(a.sf);
  const int64_t work = frames * a.total;
  const int64_t grid = (work + G - 1) / G;
  if (grid >= (int64_t(1) << 31)) return set_last_error(LORA_EINVAL, "batch too large");
  const unsigned g = (unsigned)grid;
  const uint32_t rf = (uint32_t)red_first, rc = (uint32_t)red_count;
  switch (a.sf) {
    case 7: launch_soft_frame_sf<7>(a, cfo, toff, max_amp, llr, llr_stride, work, g, st, rf, rc); break;
    case 8: launch_soft_frame_sf<8>(a, cfo, toff, max_amp, llr, llr_stride, work, g, st, rf, rc); break;
    case 9: launch_soft_frame_sf<9>(a, cfo, toff, max_amp, llr, llr_stride, work, g, st, rf, rc); break;
    case 10: launch_soft_frame_sf<10>(a, cfo, toff, max_amp, llr, llr_stride, work, g, st, rf, rc); break;
    case 11: launch_soft_frame_sf<11>(a, cfo, toff, max_amp, llr, llr_stride, work, g, st, rf, rc); break;
    case 12: launch_soft_frame_sf<12>(a, cfo, toff, max_amp, llr, llr_stride, work, g, st, rf, rc); break;
    default: return set_last_error(LORA_EINVAL, "reduced soft bits need sf in 7..12");
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_last_error(LORA_EIO, std::string("k_soft_bits_frame: ") + hipGetErrorString(e));
  return LORA_OK;
}

}  // namespace lora
