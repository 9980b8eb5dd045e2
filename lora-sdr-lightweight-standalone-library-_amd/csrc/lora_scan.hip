// lora_scan.hip — the sliding detector scan (lora_detect_scan_batch).
//
// LoRaDetector<float>::detect (LoRaDetector.hpp:39-74) on a window of N * osr samples that
// starts every `hop` samples of a continuous stream instead of every N * osr: window w of a
// row is what a LORA_MODE_RAW plan feeds for a one-symbol frame cut at sample w * hop
// ((dechirp, table index from the window start) -> window -> detect), and every output is
// bit-identical to k_detect_metrics' for that frame.  The arithmetic is lora_metrics.hip's,
// statement for statement (fft_lds, the argmax keys, the double total in bin order by one
// lane per window, detect_tail, no contraction); what is new is the addressing.
//
// A workgroup takes G = metrics_group(sf) consecutive windows of one row.  For hop < step
// they overlap: together they cover (G-1) * hop + (N-1) * osr + 1 consecutive samples, each
// of which up to step / hop windows use.  Where that segment fits, it is staged in LDS once
// with coalesced (16-byte where aligned) loads and the G leaf-ordered windows are built from
// LDS; the staging buffer is the |X|^2 array's storage, which is not written until after the
// FFT, so the scan needs not a byte of LDS more than k_detect_metrics and keeps its occupancy
// ("The sliding scan").  When hop is a multiple of osr every point any window
// uses lies on one grid of pitch osr, and only that grid is staged.  Otherwise (the segment
// does not fit, G = 1 at SF12, hop >= step) each point is loaded from global memory.
//
// k_detect_scan_acc (lora_detect_scan_acc_batch) is the same scan with the |X|^2 spectra of
// `acc` windows one symbol apart summed before the argmax and the floor, for preambled frames.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/lora_mi355x.h"
#include "lora_device.h"
#include "lora_internal.h"

#pragma clang fp contract(off)

namespace lora {
namespace {

constexpr int kThreads = 256;

struct ScanGeo {
  int64_t W;    // windows per row
  int64_t gpr;  // workgroups per row
  int64_t hop;
  // staged: samples are kept at pitch `dec` (osr when hop % osr == 0, else 1); a window is
  // hs = hop / dec staged entries after its predecessor, its points os = osr / dec apart
  int staged, dec, hs, os;
};

// Staged entries that nv consecutive windows cover.
__host__ __device__ constexpr int64_t scan_segment(int nv, int N, int64_t hs, int os) {
  return (int64_t)(nv - 1) * hs + (int64_t)(N - 1) * os + 1;
}

// One workgroup: windows w0 .. w0 + G - 1 of row blockIdx.x / gpr (LDS as k_detect_metrics:
// A [G][N] windows then spectra, M [N][G] |X|^2, K [G] argmax keys; S, the staged segment,
// aliases M).
__global__ void __launch_bounds__(kThreads)
k_detect_scan(KArgs a, ScanGeo g, lora_symbol_metrics o) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int sf = a.sf, N = a.N, G = metrics_group(sf);
  cf* A = reinterpret_cast<cf*>(smem);
  float* M = reinterpret_cast<float*>(A + (size_t)G * N);
  unsigned long long* K = reinterpret_cast<unsigned long long*>(M + (size_t)G * N);
  cf* S = reinterpret_cast<cf*>(M);
  const int tid = threadIdx.x;
  const int64_t row = (int64_t)blockIdx.x / g.gpr;
  const int64_t w0 = ((int64_t)blockIdx.x - row * g.gpr) * G;
  const int nv = g.W - w0 < G ? (int)(g.W - w0) : G;  // >= 1
  // the first sample of window w0; the last valid window ends within the row (w * hop + step
  // <= row_len for every w < W), so nothing below reads past it
  const cf* x = a.iq + row * a.frame_stride + w0 * g.hop;

  if (tid < G) K[tid] = 0;
  if (g.staged) {
    const int cnt = (int)scan_segment(nv, N, g.hs, g.os);
    if (g.dec == 1) {
      // pairs on the 16-byte grid of the address space: pair q holds segment samples
      // 2q - mis and 2q + 1 - mis; a pair that hangs over either end is loaded singly
      const int mis = (int)((reinterpret_cast<uintptr_t>(x) >> 3) & 1);
      const int pairs = (cnt + mis + 1) >> 1;
      for (int q = tid; q < pairs; q += kThreads) {
        const int s0 = 2 * q - mis;
        if (s0 >= 0 && s0 + 1 < cnt) {
          const float4 v = *reinterpret_cast<const float4*>(x + s0);
          S[s0] = cf{v.x, v.y};
          S[s0 + 1] = cf{v.z, v.w};
        } else {
          if (s0 >= 0) S[s0] = x[s0];
          if (s0 + 1 < cnt) S[s0 + 1] = x[s0 + 1];
        }
      }
    } else {
      for (int m = tid; m < cnt; m += kThreads) S[m] = x[(int64_t)m * g.dec];
    }
    __syncthreads();
  }
  // G * N is a multiple of the 256 threads (4096, or 64 N with N >= 4)
  for (int b = tid; b < G * N; b += kThreads) {
    const int sym = b >> sf, i = b & (N - 1);
    cf v{0.0f, 0.0f};
    if (sym < nv) {
      if (g.staged)
        v = S[sym * g.hs + i * g.os];
      else
        v = x[(int64_t)sym * g.hop + (int64_t)(i * a.osr)];
      if (a.dechirp) v = cmul(v, a.down[i * a.osr]);
      if (a.hann) v = cscale(v, a.win[i]);
    }
    A[sym * N + a.rev[i]] = v;
  }
  __syncthreads();  // (S is dead from here: M is written after the FFT's barriers)
  fft_lds(A, sf, G, a.tw, tid, kThreads);

  // |X|^2 of every bin and the lowest-index argmax (LoRaDetector.hpp:46-58), as
  // k_detect_metrics
  const int T = N < 64 ? N : 64;
  for (int b = tid; b < G * N; b += kThreads) {
    const int sym = b >> sf, i = b & (N - 1);
    const cf v = A[b];
    M[i * G + sym] = v.re * v.re + v.im * v.im;
    const uint64_t k = group_max(argmax_key(v, (uint32_t)i), T);
    if ((tid & (T - 1)) == 0) atomicMax(&K[sym], (unsigned long long)k);
  }
  __syncthreads();

  if (tid >= nv) return;
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
  const int64_t at = row * o.stride + w0 + tid;
  if (o.power) o.power[at] = power;
  if (o.power_avg) o.power_avg[at] = power_avg;
  if (o.f_index) o.f_index[at] = findex;
  if (o.index) o.index[at] = (uint16_t)idx;
}

// The accumulating scan (lora_detect_scan_acc_batch): output window w0 + g of the workgroup is
// the fp32 sum, oldest first, of the |X|^2 of plain windows w0 + g + q * k, q = 0 .. acc - 1.
// This is the recomputing form: the workgroup runs k_detect_scan's staging, window build and
// FFT once per q (the segment of step q begins q * step samples after the first) and keeps the
// running sums in registers - lane tid owns bins tid, tid + 256, .. of the [G][N] layout, 16 of
// them at SF >= 6 - so the LDS is k_detect_scan's to the byte.  The sums go to M after the last
// step, and the tail is the scan's on S_w.  With conj the samples are conjugated as they leave
// global memory or the staged segment.
constexpr int kAccBins = 4096 / kThreads;  // G * N <= 4096

__global__ void __launch_bounds__(kThreads)
k_detect_scan_acc(KArgs a, ScanGeo g, int acc, int conj, float* o_power, float* o_avg, uint16_t* o_index,
                  int64_t o_stride) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int sf = a.sf, N = a.N, G = metrics_group(sf);
  cf* A = reinterpret_cast<cf*>(smem);
  float* M = reinterpret_cast<float*>(A + (size_t)G * N);
  unsigned long long* K = reinterpret_cast<unsigned long long*>(M + (size_t)G * N);
  cf* S = reinterpret_cast<cf*>(M);
  const int tid = threadIdx.x;
  const int64_t row = (int64_t)blockIdx.x / g.gpr;
  const int64_t w0 = ((int64_t)blockIdx.x - row * g.gpr) * G;
  // g.W is Wa here: output window w < Wa reads plain windows up to w + (acc - 1) * k < W, each
  // of which ends within the row
  const int nv = g.W - w0 < G ? (int)(g.W - w0) : G;  // >= 1
  const cf* x0 = a.iq + row * a.frame_stride + w0 * g.hop;

  if (tid < G) K[tid] = 0;
  const int gn1 = G * N - 1;  // G * N is a power of two, and a multiple of the 256 threads
  float sum[kAccBins];
#pragma unroll
  for (int j = 0; j < kAccBins; ++j) sum[j] = 0.0f;

  for (int q = 0; q < acc; ++q) {
    const cf* x = x0 + (int64_t)q * a.step;
    if (g.staged) {
      const int cnt = (int)scan_segment(nv, N, g.hs, g.os);
      if (g.dec == 1) {
        const int mis = (int)((reinterpret_cast<uintptr_t>(x) >> 3) & 1);
        const int pairs = (cnt + mis + 1) >> 1;
        for (int p = tid; p < pairs; p += kThreads) {
          const int s0 = 2 * p - mis;
          if (s0 >= 0 && s0 + 1 < cnt) {
            const float4 v = *reinterpret_cast<const float4*>(x + s0);
            S[s0] = cf{v.x, v.y};
            S[s0 + 1] = cf{v.z, v.w};
          } else {
            if (s0 >= 0) S[s0] = x[s0];
            if (s0 + 1 < cnt) S[s0 + 1] = x[s0 + 1];
          }
        }
      } else {
        for (int m = tid; m < cnt; m += kThreads) S[m] = x[(int64_t)m * g.dec];
      }
      __syncthreads();
    }
    for (int b = tid; b < G * N; b += kThreads) {
      const int sym = b >> sf, i = b & (N - 1);
      cf v{0.0f, 0.0f};
      if (sym < nv) {
        if (g.staged)
          v = S[sym * g.hs + i * g.os];
        else
          v = x[(int64_t)sym * g.hop + (int64_t)(i * a.osr)];
        if (conj) v.im = -v.im;
        if (a.dechirp) v = cmul(v, a.down[i * a.osr]);
        if (a.hann) v = cscale(v, a.win[i]);
      }
      A[sym * N + a.rev[i]] = v;
    }
    __syncthreads();  // (S is dead from here)
    fft_lds(A, sf, G, a.tw, tid, kThreads);
    // (below SF6 G * N < 4096: the lane's later bins wrap onto its earlier ones and repeat them;
    // 0 + p is p exactly, p being a sum of squares and so never -0)
#pragma unroll
    for (int j = 0; j < kAccBins; ++j) {
      const cf v = A[(tid + j * kThreads) & gn1];
      sum[j] += v.re * v.re + v.im * v.im;
    }
    __syncthreads();  // A is rebuilt, and S restaged, by the next step
  }

  // the sums to M in the scan's [N][G] layout, then the scan's argmax over them
#pragma unroll
  for (int j = 0; j < kAccBins; ++j) {
    const int b = (tid + j * kThreads) & gn1;  // (a repeated bin stores the same value again)
    M[(b & (N - 1)) * G + (b >> sf)] = sum[j];
  }
  __syncthreads();
  const int T = N < 64 ? N : 64;
  for (int b = tid; b < G * N; b += kThreads) {
    const int sym = b >> sf, i = b & (N - 1);
    const float s = M[i * G + sym];
    const float val = (s > 0.0f) ? s : 0.0f;
    const uint64_t key = group_max(((uint64_t)__float_as_uint(val) << 32) | (uint32_t)(~(uint32_t)i), T);
    if ((tid & (T - 1)) == 0) atomicMax(&K[sym], (unsigned long long)key);
  }
  __syncthreads();

  if (tid >= nv) return;
  double total = 0.0;
#pragma unroll 8
  for (int i = 0; i < N; ++i) total += (double)M[i * G + tid];
  const uint64_t key = K[tid];
  const uint32_t idx = key_index(key);
  const float maxv = key_value(key);
  const float fundamental = sqrtf(maxv);
  const float power = 20.0f * lm_log10f(fundamental) - a.power_scale;
  const float noise = sqrtf((float)(total - (double)maxv));
  const float power_avg = 20.0f * lm_log10f(noise) - a.power_scale;
  const int64_t at = row * o_stride + w0 + tid;
  if (o_power) o_power[at] = power;
  if (o_avg) o_avg[at] = power_avg;
  if (o_index) o_index[at] = (uint16_t)idx;
}

}  // namespace

int64_t scan_windows(int64_t row_len, int64_t step, int64_t hop) {
  return row_len < step ? 0 : (row_len - step) / hop + 1;
}

int64_t scan_grid(int sf, int64_t W, int64_t rows) {
  const int G = metrics_group(sf);
  const int64_t gpr = (W + G - 1) / G, lim = int64_t(1) << 31;
  // rows * gpr < 2^31, compared through the quotient so that nothing overflows
  if (gpr == 0 || rows == 0) return 0;
  return gpr >= lim || rows > (lim - 1) / gpr ? -1 : rows * gpr;
}

int launch_detect_scan(const KArgs& a, const lora_symbol_metrics& o, int64_t rows, int64_t hop, hipStream_t st) {
  const int G = metrics_group(a.sf);
  ScanGeo g{};
  g.W = scan_windows(a.frame_len, a.step, hop);
  g.gpr = (g.W + G - 1) / G;
  const int64_t grid = scan_grid(a.sf, g.W, rows);
  if (grid <= 0) return set_last_error(LORA_EINVAL, "scan: nothing to launch or batch too large");
  g.hop = hop;
  if (G > 1 && hop < a.step) {
    g.dec = hop % a.osr == 0 ? a.osr : 1;
    g.hs = (int)(hop / g.dec);
    g.os = a.osr / g.dec;
    // the staging buffer is M's storage: G * N floats = G * N / 2 samples
    g.staged = scan_segment(G, a.N, g.hs, g.os) <= (int64_t)G * a.N / 2;
  }
  const size_t lds = (size_t)G * a.N * (sizeof(cf) + sizeof(float)) + (size_t)G * sizeof(unsigned long long);
  hipLaunchKernelGGL(k_detect_scan, dim3((unsigned)grid), dim3(kThreads), lds, st, a, g, o);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_last_error(LORA_EIO, std::string("k_detect_scan: ") + hipGetErrorString(e));
  return LORA_OK;
}

int64_t scan_acc_windows(int64_t row_len, int64_t step, int64_t hop, int64_t acc) {
  const int64_t W = scan_windows(row_len, step, hop);
  if (acc <= 1) return W;
  const int64_t Wa = W - (acc - 1) * (step / hop);
  return Wa > 0 ? Wa : 0;
}

int launch_detect_scan_acc(const KArgs& a, int64_t rows, int64_t hop, int acc, int conj, float* power,
                           float* power_avg, uint16_t* index, int64_t out_stride, hipStream_t st) {
  const int G = metrics_group(a.sf);
  ScanGeo g{};
  g.W = scan_acc_windows(a.frame_len, a.step, hop, acc);
  g.gpr = (g.W + G - 1) / G;
  const int64_t grid = scan_grid(a.sf, g.W, rows);
  if (grid <= 0) return set_last_error(LORA_EINVAL, "scan: nothing to launch or batch too large");
  g.hop = hop;
  if (G > 1 && hop < a.step) {  // as launch_detect_scan
    g.dec = hop % a.osr == 0 ? a.osr : 1;
    g.hs = (int)(hop / g.dec);
    g.os = a.osr / g.dec;
    g.staged = scan_segment(G, a.N, g.hs, g.os) <= (int64_t)G * a.N / 2;
  }
  const size_t lds = (size_t)G * a.N * (sizeof(cf) + sizeof(float)) + (size_t)G * sizeof(unsigned long long);
  hipLaunchKernelGGL(k_detect_scan_acc, dim3((unsigned)grid), dim3(kThreads), lds, st, a, g, acc, conj, power,
                     power_avg, index, out_stride);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_last_error(LORA_EIO, std::string("k_detect_scan_acc: ") + hipGetErrorString(e));
  return LORA_OK;
}

}  // namespace lora
