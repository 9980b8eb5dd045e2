// lora_find.hip — the frame finder on the device (lora_find_frames_batch).
//
// The finder's rule (include/lora_mi355x.h; lora_phy_amd/stream.py states it first) has a
// parallel half and a serial half.  Whether window w is a candidate, and the start it refines
// to, depend on the scan's outputs at w and w + k alone; the greedy pass then walks the
// candidates in order, carrying `first`.  Rejections are permanent - `first` and the pass's
// position only grow, and the tests against 0 and row_len do not depend on the pass - so the
// next frame the serial pass accepts from position p is the LOWEST w >= p that is a candidate,
// fits the row and has start >= first.  That is a find-first-set.
//
// One workgroup of kThreads takes one row, in tiles of kFindTile windows, and each tile goes
// through three stages:
//   build  each wave takes 64 consecutive windows at a time, loads the three metrics at w and
//          w + k (coalesced, all of the wave's loads issued before the first is used), and
//          leaves in LDS one 64-bit ballot word - bit set: candidate with 0 <= start <= row_len -
//          frame_len - and the 64 index values;
//   link   what the pass accepts after a frame depends on that frame alone (its end is the new
//          `first`, its window the new position), so for every set bit of the tile its successor
//          - the lowest set bit from the jump on whose start is not before this one's end - is
//          found by one lane, all bits in parallel, and left in LDS (none: the chain leaves the
//          tile);
//   walk   wave 0 finds the first frame of the tile from the state it carries (64 mask words,
//          one per lane, and a ballot to skip to the next non-empty word; the 64 starts of that
//          word, one per lane; a ballot of start >= first; the lowest set lane), then follows the
//          successors: one dependent LDS read per accepted frame.
// Every step of the walk either accepts a frame, and the successor is a later window of the
// tile, or moves the position to a later word; the position is bounded by W - k.  The stages
// are pipelined over three tile buffers: while wave 0 walks tile t, the other waves link tile
// t + 1 and build tile t + 2, with one barrier per tile.  No workgroup waits on another, nothing
// is read back from global memory, and there is no workspace.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/lora_mi355x.h"
#include "lora_internal.h"

namespace lora {
namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kFindTile = 4096;             // windows per tile
constexpr int kTileWords = kFindTile / 64;  // ballot words per tile

struct FindArgs {
  const float* power;
  const float* power_avg;
  const uint16_t* index;
  const int64_t* first;  // [rows] or null
  int64_t* starts;       // [rows][capacity]
  int32_t* count;        // [rows]
  int64_t* end;          // [rows]
  int64_t stride, capacity;
  int64_t n;             // W - k: windows the pass may test (may be <= 0)
  int64_t hop, osr, half_step, frame_len;
  int64_t last_start;    // row_len - frame_len: the last start that fits (may be < 0)
  int64_t lead_q;        // frame_len - step / 2 = lead_q * hop + lead_r, 0 <= lead_r < hop
  int lead_r, hop32;
  int k, N, sw0, dsync;  // dsync = (sw1 - sw0) mod N
  float thresh;
};

struct Tile {
  unsigned long long mask[kTileWords];
  uint16_t index[kFindTile];
};
constexpr unsigned kNoSucc = 0xFFFFu;  // in a tile's successor array: the chain leaves the tile

// d folded to [-N/2, N/2) and the refined start of window w whose peak is `idx`.
__device__ __forceinline__ int64_t refined_start(const FindArgs& a, int64_t w, int idx) {
  int d = (idx - a.sw0) & (a.N - 1);
  if (d >= a.N / 2) d -= a.N;
  return w * a.hop - (int64_t)d * a.osr;
}

// Where the pass goes on after accepting window w with start s: the smallest w' > w with
// w' * hop >= s + frame_len - step / 2.  That bound is w * hop + (s - w * hop) + lead_q * hop +
// lead_r, and |s - w * hop| <= step / 2, so the one division is of 32-bit values.
__device__ __forceinline__ int64_t next_window(const FindArgs& a, int64_t w, int64_t s) {
  const int c = a.lead_r + (int)(s - w * a.hop);
  const int64_t wn = w + a.lead_q + (c / a.hop32 + (c % a.hop32 > 0));
  return wn > w + 1 ? wn : w + 1;
}

// Words word0, word0 + nwaves, .. of the tile that starts at window `base` with nt windows,
// by the calling wave: at most kWordsPerWave of them (nwaves >= kWaves - 1).  All loads of the
// wave's words are issued before the first is used, so a tile costs one trip to memory, not
// one per word.
constexpr int kWordsPerWave = (kTileWords + kWaves - 2) / (kWaves - 1);

__device__ __forceinline__ void build_tile(const FindArgs& a, const float* pw, const float* pa, const uint16_t* ix,
                                           Tile& t, int64_t base, int nt, int word0, int nwaves, int lane) {
  const int words = (nt + 63) >> 6;
  float p0[kWordsPerWave], f0[kWordsPerWave], p1[kWordsPerWave], f1[kWordsPerWave];
  int i0[kWordsPerWave], i1[kWordsPerWave];
#pragma unroll
  for (int u = 0; u < kWordsPerWave; ++u) {
    const int rel = (word0 + u * nwaves) * 64 + lane;
    p0[u] = f0[u] = p1[u] = f1[u] = 0.0f;
    i0[u] = i1[u] = 0;
    if (rel < nt) {
      const int64_t w = base + rel;  // w + k < W
      i0[u] = ix[w];
      i1[u] = ix[w + a.k];
      p0[u] = pw[w];
      f0[u] = pa[w];
      p1[u] = pw[w + a.k];
      f1[u] = pa[w + a.k];
    }
  }
#pragma unroll
  for (int u = 0; u < kWordsPerWave; ++u) {
    const int word = word0 + u * nwaves, rel = word * 64 + lane;
    if (word >= words) break;
    const int64_t start = refined_start(a, base + rel, i0[u]);
    const bool bit = rel < nt && p0[u] - f0[u] >= a.thresh && p1[u] - f1[u] >= a.thresh &&
                     ((i1[u] - i0[u]) & (a.N - 1)) == a.dsync && start >= 0 && start <= a.last_start;
    const unsigned long long m = __ballot(bit);
    t.index[rel] = (uint16_t)i0[u];
    if (lane == 0) t.mask[word] = m;
  }
}

struct Pass {
  int64_t first, w;  // no frame starts before `first`; the next window to test
  int64_t cnt;
};

// v of lane l, the same l in every lane.
__device__ __forceinline__ unsigned long long lane_value(unsigned long long v, int l) {
  l = __builtin_amdgcn_readfirstlane(l);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
  return ((unsigned long long)hi << 32) | lo;
}

// The successor of every set bit of a built tile (windows wave0 * 64 + lane, + nwaves * 64, ..):
// succ[rel] = the tile-relative window the pass accepts after accepting rel, or kNoSucc.
__device__ __forceinline__ void link_tile(const FindArgs& a, const Tile& t, uint16_t* succ, int64_t base, int nt,
                                          int wave0, int nwaves, int lane) {
  const int words = (nt + 63) >> 6;
  for (int rel = wave0 * 64 + lane; rel < nt; rel += nwaves * 64) {
    if (((t.mask[rel >> 6] >> (rel & 63)) & 1ull) == 0ull) continue;
    const int64_t w = base + rel, s = refined_start(a, w, t.index[rel]), first = s + a.frame_len;
    const int64_t wn = next_window(a, w, s);  // > w
    unsigned res = kNoSucc;
    if (wn < base + nt) {
      int word = (int)(wn - base) >> 6;
      unsigned long long b = t.mask[word] & (~0ull << ((int)(wn - base) & 63));
      for (;;) {  // every turn clears a bit or moves to the next word
        while (b != 0ull && res == kNoSucc) {
          const int u = word * 64 + __ffsll((long long)b) - 1;
          if (refined_start(a, base + u, t.index[u]) >= first) res = (unsigned)u;
          b &= b - 1;
        }
        if (res != kNoSucc || ++word >= words) break;
        b = t.mask[word];
      }
    }
    succ[rel] = (uint16_t)res;
  }
}

// The first window of the tile the pass accepts from its state p (tile-relative), or -1 with
// the position moved to the tile's end.  One whole wave, uniform state; p.w >= base.
__device__ __forceinline__ int first_in_tile(const FindArgs& a, const Tile& t, int64_t base, int nt, Pass& p,
                                             int lane) {
  const int words = (nt + 63) >> 6;
  const int64_t stop = base + nt;
  while (p.w < stop) {
    // mask words wb .. wb + 63, one per lane, wb the position's word; the block ends at `bend`
    const int wb = (int)(p.w - base) >> 6;
    const unsigned long long m = wb + lane < words ? t.mask[wb + lane] : 0ull;
    const int64_t bfull = base + (int64_t)(wb + 64) * 64;
    const int64_t bend = bfull < stop ? bfull : stop;  // > p.w
    while (p.w < bend) {
      // the next non-empty word of the block from the position on (bits below it cleared)
      const int rel = (int)(p.w - base), j0 = (rel >> 6) - wb;
      unsigned long long mm = lane < j0 ? 0ull : m;
      if (lane == j0) mm &= ~0ull << (rel & 63);
      const unsigned long long nz = __ballot(mm != 0ull);
      if (nz == 0ull) {
        p.w = bend;
        break;
      }
      const int j = __ffsll((long long)nz) - 1;
      const unsigned long long bits = lane_value(mm, j);
      const int word = wb + j;
      // lane l: window word * 64 + l of the tile
      const int64_t start = refined_start(a, base + (int64_t)word * 64 + lane, t.index[word * 64 + lane]);
      const unsigned long long ok = __ballot(((bits >> lane) & 1ull) != 0ull && start >= p.first);
      if (ok != 0ull) return word * 64 + __ffsll((long long)ok) - 1;  // >= p.w - base
      const int64_t nw = base + (int64_t)(word + 1) * 64;  // > p.w, <= bfull
      p.w = nw < stop ? nw : stop;
    }
  }
  return -1;
}

// The greedy pass over one built and linked tile, by one whole wave (all 64 lanes, uniform
// state): the first frame by search, the rest by their successors.
__device__ __forceinline__ void walk_tile(const FindArgs& a, const Tile& t, const uint16_t* succ, int64_t base,
                                          int nt, int64_t* starts, Pass& p, int lane) {
  int rel = first_in_tile(a, t, base, nt, p, lane);
  if (rel < 0) return;
  const int64_t stop = base + nt;
  for (;;) {  // rel grows with every turn and stays below nt
    const int64_t w = base + rel, s = refined_start(a, w, t.index[rel]);
    const unsigned nx = succ[rel];
    if (lane == 0 && p.cnt < a.capacity) starts[p.cnt] = s;
    ++p.cnt;
    p.first = s + a.frame_len;
    if (nx == kNoSucc) {
      // nothing more in this tile: on from the jump, or from the next tile if that is later
      const int64_t wn = next_window(a, w, s);
      p.w = wn > stop ? wn : stop;
      return;
    }
    rel = (int)nx;
  }
}

__global__ void __launch_bounds__(kThreads) k_find_frames(FindArgs a) {
  __shared__ Tile tiles[3];
  __shared__ uint16_t succ[2][kFindTile];
  __shared__ int64_t done;  // the row's count, for the fill
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row = blockIdx.x;
  const float* pw = a.power + row * a.stride;
  const float* pa = a.power_avg + row * a.stride;
  const uint16_t* ix = a.index + row * a.stride;
  int64_t* starts = a.starts + row * a.capacity;

  Pass p;
  p.first = a.first ? a.first[row] : 0;
  p.cnt = 0;
  // ceil(max(first - step / 2, 0) / hop), kept within the windows there are
  const int64_t lead = p.first > a.half_step ? p.first - a.half_step : 0;
  p.w = lead / a.hop + (lead % a.hop != 0);
  const int64_t n = a.n > 0 ? a.n : 0;
  if (p.w > n) p.w = n;

  const int64_t t0 = p.w / kFindTile, t1 = (n + kFindTile - 1) / kFindTile;  // tiles t0 .. t1 - 1
  const auto windows = [n](int64_t t) {  // of tile t < t1
    const int64_t left = n - t * kFindTile;
    return left < kFindTile ? (int)left : kFindTile;
  };
  // tile t is built into tiles[t % 3] and linked into succ[t & 1]
  if (t0 < t1) build_tile(a, pw, pa, ix, tiles[t0 % 3], t0 * kFindTile, windows(t0), wave, kWaves, lane);
  __syncthreads();
  if (t0 < t1) {
    link_tile(a, tiles[t0 % 3], succ[t0 & 1], t0 * kFindTile, windows(t0), wave, kWaves, lane);
    if (t0 + 1 < t1)
      build_tile(a, pw, pa, ix, tiles[(t0 + 1) % 3], (t0 + 1) * kFindTile, windows(t0 + 1), wave, kWaves, lane);
  }
  __syncthreads();
  for (int64_t t = t0; t < t1; ++t) {
    if (wave == 0) {
      walk_tile(a, tiles[t % 3], succ[t & 1], t * kFindTile, windows(t), starts, p, lane);
    } else {
      // (tiles[(t + 2) % 3] was last read while tile t - 1 was walked, succ[(t + 1) & 1] too)
      if (t + 2 < t1)
        build_tile(a, pw, pa, ix, tiles[(t + 2) % 3], (t + 2) * kFindTile, windows(t + 2), wave - 1, kWaves - 1,
                   lane);
      if (t + 1 < t1)
        link_tile(a, tiles[(t + 1) % 3], succ[(t + 1) & 1], (t + 1) * kFindTile, windows(t + 1), wave - 1,
                  kWaves - 1, lane);
    }
    __syncthreads();
  }
  if (tid == 0) {
    done = p.cnt;
    a.count[row] = (int32_t)p.cnt;  // cnt <= n < 2^31
    a.end[row] = p.first;
  }
  __syncthreads();
  for (int64_t i = (done < a.capacity ? done : a.capacity) + tid; i < a.capacity; i += kThreads) starts[i] = -1;
}

// ---------------------------------------------------------------------------------------------
// Frames that state their own length: the candidates are listed, their headers decoded
// (lora_decode_frame_batch), and the pass runs over the slots whose header is good.
// ---------------------------------------------------------------------------------------------

// lora_find_candidates_batch: the candidate rule and refinement of build_tile, listed instead of
// walked.  A candidate is eligible when its start lies in 0 .. last_start (here: the header's ten
// symbols fit the row); it is listed unless its start equals the last listed one - which is the
// start of the eligible candidate before it, listed or not, so the test is local.  One workgroup
// takes a row, kThreads windows at a time: a ballot of the eligible, each eligible lane looks up
// its predecessor's start (this wave's ballot, the waves before, the turn before), a ballot of
// the listed, and the slot is the count so far plus the set bits below.  FindArgs as the finder's,
// `first`, `end` and the jump's fields unused.
__global__ void __launch_bounds__(kThreads) k_find_candidates(FindArgs a) {
  __shared__ unsigned long long elig[kWaves], listed[kWaves];
  __shared__ int64_t st[kThreads];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row = blockIdx.x;
  const float* pw = a.power + row * a.stride;
  const float* pa = a.power_avg + row * a.stride;
  const uint16_t* ix = a.index + row * a.stride;
  int64_t* starts = a.starts + row * a.capacity;
  const unsigned long long below = (1ull << lane) - 1ull;
  // uniform over the workgroup: listed so far, and the last eligible start of the turns before
  int64_t cnt = 0, prev = -1;  // (no eligible start is negative)
  for (int64_t base = 0; base < a.n; base += kThreads) {
    const int64_t w = base + tid;
    bool el = false;
    int64_t s = -1;
    if (w < a.n) {  // w + k < W
      const int i0 = ix[w], i1 = ix[w + a.k];
      const float p0 = pw[w], f0 = pa[w], p1 = pw[w + a.k], f1 = pa[w + a.k];
      s = refined_start(a, w, i0);
      el = p0 - f0 >= a.thresh && p1 - f1 >= a.thresh && ((i1 - i0) & (a.N - 1)) == a.dsync && s >= 0 &&
           s <= a.last_start;
    }
    const unsigned long long m = __ballot(el);
    st[tid] = s;
    if (lane == 0) elig[wave] = m;
    __syncthreads();
    bool list = false;
    if (el) {
      int64_t ps = prev;
      if (m & below) {
        ps = st[wave * 64 + 63 - __clzll((long long)(m & below))];
      } else {
        int v = wave - 1;
        while (v >= 0 && elig[v] == 0ull) --v;
        if (v >= 0) ps = st[v * 64 + 63 - __clzll((long long)elig[v])];
      }
      list = ps != s;
    }
    const unsigned long long ml = __ballot(list);
    if (lane == 0) listed[wave] = ml;
    __syncthreads();
    int before = 0, total = 0, lastw = -1;
    for (int v = 0; v < kWaves; ++v) {
      const int c = __popcll(listed[v]);
      if (v < wave) before += c;
      total += c;
      if (elig[v] != 0ull) lastw = v;
    }
    if (list) {
      const int64_t pos = cnt + before + __popcll(ml & below);
      if (pos < a.capacity) starts[pos] = s;
    }
    if (lastw >= 0) prev = st[lastw * 64 + 63 - __clzll((long long)elig[lastw])];
    cnt += total;
    __syncthreads();  // st, elig and listed are rewritten by the next turn
  }
  if (tid == 0) a.count[row] = (int32_t)cnt;  // cnt <= n < 2^31
  for (int64_t i = (cnt < a.capacity ? cnt : a.capacity) + tid; i < a.capacity; i += kThreads) starts[i] = -1;
}

// lora_select_frames_batch: the greedy pass over a row's slots, in slot order.  What makes a slot
// eligible - a good header, a frame no longer than max_symbols that fits the row - does not
// depend on the pass, so the workgroup tests kSelThreads slots at a time in parallel and one
// lane walks the set bits alone, carrying `first`.
constexpr int kSelThreads = 256;
struct SelectArgs {
  const int64_t* starts;   // [rows][slots]
  const int32_t* status;   // [rows][slots]
  const int32_t* nsym;     // [rows][slots]
  const int64_t* first;    // [rows] or null
  int64_t slots, row_len, step, capacity;
  int max_symbols;
  int64_t* out_starts;     // [rows][capacity]
  int32_t* out_nsym;       // [rows][capacity]
  int32_t* count;          // [rows]
  int64_t* end;            // [rows]
  // lora_select_preamble_batch: samples a frame takes beyond its (2 + nsym) symbols, and one
  // word per slot carried to the accepted slot (both null: none)
  int64_t tail;
  const int32_t* word;     // [rows][slots] or null
  int32_t* out_word;       // [rows][capacity] or null
};

__global__ void __launch_bounds__(kSelThreads) k_select_frames(SelectArgs a) {
  __shared__ unsigned long long elig[kSelThreads / 64];
  __shared__ int64_t st[kSelThreads];
  __shared__ int32_t ns[kSelThreads];
  __shared__ int64_t s_first, s_cnt;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row = blockIdx.x;
  int64_t* out_starts = a.out_starts + row * a.capacity;
  int32_t* out_nsym = a.out_nsym + row * a.capacity;
  int32_t* out_word = a.out_word ? a.out_word + row * a.capacity : nullptr;
  if (tid == 0) {
    s_first = a.first ? a.first[row] : 0;
    s_cnt = 0;
  }
  // With a word to carry, the serial lane leaves in ns[i] of every slot it stores, in place of
  // the nsym it has used, -1 - (the slot's output position - cnt0), cnt0 the count before this
  // turn; after the turn's barrier lane i, which holds slot i's word, stores it there.  (No LDS
  // beyond the pass's own; an eligible slot's nsym is never negative.  A turn stores at most
  // kSelThreads slots, so the mark lies in -kSelThreads .. -1 and the position it stands for in
  // cnt0 .. cnt0 + kSelThreads - 1, below capacity because only stored slots are marked.)
  int64_t cnt0 = 0;
  for (int64_t base = 0; base < a.slots; base += kSelThreads) {
    const int64_t j = base + tid;
    bool el = false;
    int64_t s = -1;
    int32_t n = 0, wv = 0;
    if (j < a.slots) {
      s = a.starts[row * a.slots + j];
      n = a.nsym[row * a.slots + j];
      if (a.word) wv = a.word[row * a.slots + j];
      el = a.status[row * a.slots + j] == LORA_FRAME_OK && n >= 0 && n <= a.max_symbols && s >= 0 &&
           s <= a.row_len - (2 + (int64_t)n) * a.step - a.tail;
    }
    const unsigned long long m = __ballot(el);
    st[tid] = s;
    ns[tid] = n;
    if (lane == 0) elig[wave] = m;
    __syncthreads();
    if (tid == 0) {
      int64_t first = s_first, cnt = s_cnt;
      for (int v = 0; v < kSelThreads / 64; ++v) {
        for (unsigned long long b = elig[v]; b != 0ull; b &= b - 1) {
          const int i = v * 64 + __ffsll((long long)b) - 1;
          if (st[i] < first) continue;
          const int32_t ni = ns[i];
          if (cnt < a.capacity) {
            out_starts[cnt] = st[i];
            out_nsym[cnt] = ni;
            if (out_word) ns[i] = -1 - (int32_t)(cnt - s_cnt);
          }
          ++cnt;
          first = st[i] + (2 + (int64_t)ni) * a.step + a.tail;
        }
      }
      s_first = first;
      s_cnt = cnt;
    }
    __syncthreads();
    if (out_word) {
      if (el && ns[tid] < 0) out_word[cnt0 + (-1 - ns[tid])] = wv;
      cnt0 = s_cnt;  // (rewritten by lane 0 only after the next turn's first barrier)
    }
  }
  __syncthreads();  // (no slots: s_first and s_cnt as tid 0 set them)
  const int64_t done = s_cnt;
  if (tid == 0) {
    a.count[row] = (int32_t)done;  // done <= slots < 2^31
    a.end[row] = s_first;
  }
  for (int64_t i = (done < a.capacity ? done : a.capacity) + tid; i < a.capacity; i += kSelThreads) {
    out_starts[i] = -1;
    out_nsym[i] = 0;
    if (out_word) out_word[i] = 0;
  }
}

// ---------------------------------------------------------------------------------------------
// Preambled frames: lora_find_preamble_batch.  The rule (include/lora_mi355x.h) reads the up scan
// at u = w - (2 + m) * k and the down scan at w - k, w and w + k, so like the candidate list it
// is parallel over w but for the local "differs from the previous passing pair" test: the
// geometry, ballots and prefix count are k_find_candidates'.
// ---------------------------------------------------------------------------------------------
struct PreambleArgs {
  const float *up_power, *up_avg, *dn_power, *dn_avg;
  const uint16_t *up_index, *dn_index;
  int64_t up_stride, dn_stride;
  int64_t w_lo, w_hi;  // down windows w_lo <= w < w_hi are tested (w_hi <= w_lo: none)
  int64_t lag;         // (2 + m) * k
  int64_t hop, osr, two_step, capacity;
  int64_t last_start;  // row_len - 10 * step - tail (may be < 0)
  int64_t* starts;     // [rows][capacity]
  int32_t* cfo;        // [rows][capacity]
  int32_t* count;      // [rows]
  int k, N, max_cfo;
  float thresh_up, thresh_dn;
};

__global__ void __launch_bounds__(kThreads) k_find_preamble(PreambleArgs a) {
  __shared__ unsigned long long elig[kWaves], listed[kWaves];
  __shared__ int64_t st[kThreads];
  __shared__ int32_t cf_[kThreads];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row = blockIdx.x;
  const float* up = a.up_power + row * a.up_stride;
  const float* ua = a.up_avg + row * a.up_stride;
  const uint16_t* ui = a.up_index + row * a.up_stride;
  const float* dp = a.dn_power + row * a.dn_stride;
  const float* da = a.dn_avg + row * a.dn_stride;
  const uint16_t* di = a.dn_index + row * a.dn_stride;
  int64_t* starts = a.starts + row * a.capacity;
  int32_t* cfo = a.cfo + row * a.capacity;
  const unsigned long long below = (1ull << lane) - 1ull;
  int64_t cnt = 0, prev_s = -1;  // (no passing start is negative)
  int32_t prev_c = 0;
  for (int64_t base = a.w_lo; base < a.w_hi; base += kThreads) {
    const int64_t w = base + tid;
    bool el = false;
    int64_t s = -1;
    int32_t c = 0;
    if (w < a.w_hi) {  // w - k >= 0, w + k < Wd, 0 <= w - lag < Wu
      const int64_t u = w - a.lag;
      const float p0 = dp[w], f0 = da[w], pm = dp[w - a.k], pp = dp[w + a.k];
      const float p1 = up[u], f1 = ua[u];
      const int iu = ui[u], id = di[w];
      int sum = (iu + id) & (a.N - 1);
      if (sum >= a.N / 2) sum -= a.N;
      const int d = sum >> 1;  // floor
      c = (iu - d) & (a.N - 1);
      if (c >= a.N / 2) c -= a.N;
      s = w * a.hop - (int64_t)d * a.osr - a.two_step;
      el = p0 - f0 >= a.thresh_dn && p1 - f1 >= a.thresh_up && p0 >= pm && p0 > pp &&
           (c < 0 ? -c : c) <= a.max_cfo && s >= 0 && s <= a.last_start;
    }
    const unsigned long long m = __ballot(el);
    st[tid] = s;
    cf_[tid] = c;
    if (lane == 0) elig[wave] = m;
    __syncthreads();
    bool list = false;
    if (el) {
      int64_t ps = prev_s;
      int32_t pc = prev_c;
      int at = -1;
      if (m & below) {
        at = wave * 64 + 63 - __clzll((long long)(m & below));
      } else {
        int v = wave - 1;
        while (v >= 0 && elig[v] == 0ull) --v;
        if (v >= 0) at = v * 64 + 63 - __clzll((long long)elig[v]);
      }
      if (at >= 0) {
        ps = st[at];
        pc = cf_[at];
      }
      list = ps != s || pc != c;
    }
    const unsigned long long ml = __ballot(list);
    if (lane == 0) listed[wave] = ml;
    __syncthreads();
    int before = 0, total = 0, lastw = -1;
    for (int v = 0; v < kWaves; ++v) {
      const int n = __popcll(listed[v]);
      if (v < wave) before += n;
      total += n;
      if (elig[v] != 0ull) lastw = v;
    }
    if (list) {
      const int64_t pos = cnt + before + __popcll(ml & below);
      if (pos < a.capacity) {
        starts[pos] = s;
        cfo[pos] = c;
      }
    }
    if (lastw >= 0) {
      const int at = lastw * 64 + 63 - __clzll((long long)elig[lastw]);
      prev_s = st[at];
      prev_c = cf_[at];
    }
    cnt += total;
    __syncthreads();  // st, cf_, elig and listed are rewritten by the next turn
  }
  if (tid == 0) a.count[row] = (int32_t)cnt;  // cnt <= Wd < 2^31
  for (int64_t i = (cnt < a.capacity ? cnt : a.capacity) + tid; i < a.capacity; i += kThreads) {
    starts[i] = -1;
    cfo[i] = 0;
  }
}

}  // namespace
}  // namespace lora

using lora::set_last_error;

extern "C" {

int64_t lora_find_candidates_batch(const lora_find_params* p, const float* power, const float* power_avg,
                                   const uint16_t* index, int64_t rows, int64_t W, int64_t stride,
                                   int64_t row_len, int64_t capacity, int64_t* starts, int32_t* count,
                                   void* stream) {
  if (!p) return set_last_error(LORA_EINVAL, "null params");
  if (p->sf < 6 || p->sf > 12) return set_last_error(LORA_EINVAL, "the frame finder needs SF 6-12");
  if (p->osr < 1 || p->osr > (1u << 16)) return set_last_error(LORA_EINVAL, "osr must be in 1..65536");
  const int64_t N = int64_t(1) << p->sf, step = N * (int64_t)p->osr;
  if (p->hop < 1 || step % p->hop != 0 || step / p->hop < 2)
    return set_last_error(LORA_EINVAL, "hop must divide step = N * osr at least twice");
  if (rows < 0 || W < 0 || stride < 0 || row_len < 0 || capacity < 0)
    return set_last_error(LORA_EINVAL, "negative rows / W / stride / row_len / capacity");
  if (W >= (int64_t(1) << 31)) return set_last_error(LORA_EINVAL, "W must be < 2^31");
  if (rows >= (int64_t(1) << 31)) return set_last_error(LORA_EINVAL, "batch too large");
  if (rows > 1 && stride < W) return set_last_error(LORA_EINVAL, "stride smaller than windows per row");
  if (rows == 0) return 0;
  if (!count || (capacity > 0 && !starts)) return set_last_error(LORA_EINVAL, "null output");
  const int64_t k = step / p->hop;
  if (W > k && (!power || !power_avg || !index)) return set_last_error(LORA_EINVAL, "null metrics");
  lora::FindArgs a{};
  a.power = power;
  a.power_avg = power_avg;
  a.index = index;
  a.starts = starts;
  a.count = count;
  a.stride = stride;
  a.capacity = capacity;
  a.n = W - k;
  a.hop = p->hop;
  a.osr = p->osr;
  a.half_step = step / 2;
  a.frame_len = 10 * step;  // the two sync symbols and the header's eight
  a.last_start = row_len - a.frame_len;
  a.k = (int)k;
  a.N = (int)N;
  const int sync = (int)(p->sync & 0xFFu);
  a.sw0 = (sync >> 4) << (p->sf - 4);
  const int sw1 = (sync & 15) << (p->sf - 4);
  a.dsync = (sw1 - a.sw0) & (a.N - 1);
  a.thresh = p->thresh_db;
  lora::DeviceGuard guard(p->device);
  if (guard.err != hipSuccess) return lora::hip_error("find device", guard.err);
  hipLaunchKernelGGL(lora::k_find_candidates, dim3((unsigned)rows), dim3(lora::kThreads), 0,
                     static_cast<hipStream_t>(stream), a);
  const hipError_t e = hipGetLastError();
  return e != hipSuccess ? lora::hip_error("k_find_candidates", e) : rows;
}

int64_t lora_find_preamble_batch(const lora_preamble_params* p, const float* up_power, const float* up_avg,
                                 const uint16_t* up_index, int64_t Wu, int64_t up_stride, const float* dn_power,
                                 const float* dn_avg, const uint16_t* dn_index, int64_t Wd, int64_t dn_stride,
                                 int64_t rows, int64_t row_len, int64_t capacity, int64_t* starts,
                                 int32_t* cfo_bins, int32_t* count, void* stream) {
  if (!p) return set_last_error(LORA_EINVAL, "null params");
  if (p->sf < 7 || p->sf > 12) return set_last_error(LORA_EINVAL, "the preamble finder needs SF 7-12");
  if (p->osr < 1 || p->osr > (1u << 16)) return set_last_error(LORA_EINVAL, "osr must be in 1..65536");
  const int64_t N = int64_t(1) << p->sf, step = N * (int64_t)p->osr;
  if (p->hop < 1 || step % p->hop != 0 || step / p->hop < 4)
    return set_last_error(LORA_EINVAL, "hop must divide step = N * osr at least four times");
  if (p->acc_up < 2 || p->acc_up > 8) return set_last_error(LORA_EINVAL, "acc_up must be in 2..8");
  if (p->max_cfo_bins < 0 || p->max_cfo_bins > N / 4 - 1)
    return set_last_error(LORA_EINVAL, "max_cfo_bins must be in 0 .. N/4 - 1");
  if (rows < 0 || Wu < 0 || Wd < 0 || up_stride < 0 || dn_stride < 0 || row_len < 0 || capacity < 0)
    return set_last_error(LORA_EINVAL, "negative rows / W / stride / row_len / capacity");
  if (Wu >= (int64_t(1) << 31) || Wd >= (int64_t(1) << 31)) return set_last_error(LORA_EINVAL, "W must be < 2^31");
  if (rows >= (int64_t(1) << 31)) return set_last_error(LORA_EINVAL, "batch too large");
  if (rows > 1 && (up_stride < Wu || dn_stride < Wd))
    return set_last_error(LORA_EINVAL, "stride smaller than windows per row");
  if (rows == 0) return 0;
  if (!count || (capacity > 0 && (!starts || !cfo_bins))) return set_last_error(LORA_EINVAL, "null output");
  const int64_t k = step / p->hop, lag = (2 + (int64_t)p->acc_up) * k;
  const int64_t w_hi = Wd - k < Wu + lag ? Wd - k : Wu + lag;
  if (w_hi > lag && (!up_power || !up_avg || !up_index || !dn_power || !dn_avg || !dn_index))
    return set_last_error(LORA_EINVAL, "null metrics");
  lora::PreambleArgs a{};
  a.up_power = up_power;
  a.up_avg = up_avg;
  a.up_index = up_index;
  a.dn_power = dn_power;
  a.dn_avg = dn_avg;
  a.dn_index = dn_index;
  a.up_stride = up_stride;
  a.dn_stride = dn_stride;
  a.w_lo = lag;
  a.w_hi = w_hi;
  a.lag = lag;
  a.hop = p->hop;
  a.osr = p->osr;
  a.two_step = 2 * step;
  a.capacity = capacity;
  a.last_start = row_len - 10 * step - 9 * step / 4;
  a.starts = starts;
  a.cfo = cfo_bins;
  a.count = count;
  a.k = (int)k;
  a.N = (int)N;
  a.max_cfo = p->max_cfo_bins;
  a.thresh_up = p->thresh_up_db;
  a.thresh_dn = p->thresh_dn_db;
  lora::DeviceGuard guard(p->device);
  if (guard.err != hipSuccess) return lora::hip_error("find device", guard.err);
  hipLaunchKernelGGL(lora::k_find_preamble, dim3((unsigned)rows), dim3(lora::kThreads), 0,
                     static_cast<hipStream_t>(stream), a);
  const hipError_t e = hipGetLastError();
  return e != hipSuccess ? lora::hip_error("k_find_preamble", e) : rows;
}

// lora_select_frames_batch (tail == 0, no words) and lora_select_preamble_batch: one validation,
// one kernel
static int64_t select_entry(const int64_t* cand_starts, const int32_t* cand_word, const int32_t* status,
                            const int32_t* nsym, int64_t rows, int64_t slots, const int64_t* first, int64_t row_len,
                            int64_t step, int64_t tail, int64_t max_symbols, int64_t capacity, int64_t* starts,
                            int32_t* out_word, int32_t* out_nsym, int32_t* count, int64_t* end, int device,
                            void* stream);

int64_t lora_select_preamble_batch(const int64_t* cand_starts, const int32_t* cand_word, const int32_t* status,
                                   const int32_t* nsym, int64_t rows, int64_t slots, const int64_t* first,
                                   int64_t row_len, int64_t step, int64_t tail, int64_t max_symbols,
                                   int64_t capacity, int64_t* starts, int32_t* out_word, int32_t* out_nsym,
                                   int32_t* count, int64_t* end, int device, void* stream) {
  if (tail < 0) return set_last_error(LORA_EINVAL, "tail must be >= 0");
  if (rows > 0 && slots > 0 && capacity > 0 && (cand_word == nullptr) != (out_word == nullptr))
    return set_last_error(LORA_EINVAL, "cand_word and out_word go together");
  return select_entry(cand_starts, cand_word, status, nsym, rows, slots, first, row_len, step, tail, max_symbols,
                      capacity, starts, out_word, out_nsym, count, end, device, stream);
}

int64_t lora_select_frames_batch(const int64_t* cand_starts, const int32_t* status, const int32_t* nsym,
                                 int64_t rows, int64_t slots, const int64_t* first, int64_t row_len, int64_t step,
                                 int64_t max_symbols, int64_t capacity, int64_t* starts, int32_t* out_nsym,
                                 int32_t* count, int64_t* end, int device, void* stream) {
  return select_entry(cand_starts, nullptr, status, nsym, rows, slots, first, row_len, step, 0, max_symbols, capacity,
                      starts, nullptr, out_nsym, count, end, device, stream);
}

static int64_t select_entry(const int64_t* cand_starts, const int32_t* cand_word, const int32_t* status,
                            const int32_t* nsym, int64_t rows, int64_t slots, const int64_t* first, int64_t row_len,
                            int64_t step, int64_t tail, int64_t max_symbols, int64_t capacity, int64_t* starts,
                            int32_t* out_word, int32_t* out_nsym, int32_t* count, int64_t* end, int device,
                            void* stream) {
  if (rows < 0 || slots < 0 || row_len < 0 || capacity < 0 || step < 1 || max_symbols < 0)
    return set_last_error(LORA_EINVAL, "negative rows / slots / row_len / capacity / max_symbols, or step < 1");
  if (rows >= (int64_t(1) << 31) || slots >= (int64_t(1) << 31) || max_symbols >= (int64_t(1) << 31))
    return set_last_error(LORA_EINVAL, "batch too large");
  if (rows == 0) return 0;
  if (!count || !end || (capacity > 0 && (!starts || !out_nsym))) return set_last_error(LORA_EINVAL, "null output");
  if (slots > 0 && (!cand_starts || !status || !nsym)) return set_last_error(LORA_EINVAL, "null slots");
  lora::SelectArgs a{};
  a.tail = tail;
  a.word = slots > 0 ? cand_word : nullptr;
  a.out_word = capacity > 0 ? out_word : nullptr;
  a.starts = cand_starts;
  a.status = status;
  a.nsym = nsym;
  a.first = first;
  a.slots = slots;
  a.row_len = row_len;
  a.step = step;
  a.capacity = capacity;
  a.max_symbols = (int)max_symbols;
  a.out_starts = starts;
  a.out_nsym = out_nsym;
  a.count = count;
  a.end = end;
  lora::DeviceGuard guard(device);
  if (guard.err != hipSuccess) return lora::hip_error("select device", guard.err);
  hipLaunchKernelGGL(lora::k_select_frames, dim3((unsigned)rows), dim3(lora::kSelThreads), 0,
                     static_cast<hipStream_t>(stream), a);
  const hipError_t e = hipGetLastError();
  return e != hipSuccess ? lora::hip_error("k_select_frames", e) : rows;
}

int64_t lora_find_frames_tile(void) { return lora::kFindTile; }

int64_t lora_find_frames_batch(const lora_find_params* p, const float* power, const float* power_avg,
                               const uint16_t* index, int64_t rows, int64_t W, int64_t stride, const int64_t* first,
                               int64_t row_len, int64_t capacity, int64_t* starts, int32_t* count, int64_t* end,
                               void* stream) {
  if (!p) return set_last_error(LORA_EINVAL, "null params");
  if (p->sf < 6 || p->sf > 12) return set_last_error(LORA_EINVAL, "the frame finder needs SF 6-12");
  if (p->osr < 1 || p->osr > (1u << 16)) return set_last_error(LORA_EINVAL, "osr must be in 1..65536");
  const int64_t N = int64_t(1) << p->sf, step = N * (int64_t)p->osr;
  if (p->hop < 1 || step % p->hop != 0 || step / p->hop < 2)
    return set_last_error(LORA_EINVAL, "hop must divide step = N * osr at least twice");
  if (p->frame_symbols < 0 || p->frame_symbols >= (int64_t(1) << 31))
    return set_last_error(LORA_EINVAL, "frame_symbols must be in 0 .. 2^31 - 1");
  if (rows < 0 || W < 0 || stride < 0 || row_len < 0 || capacity < 0)
    return set_last_error(LORA_EINVAL, "negative rows / W / stride / row_len / capacity");
  if (W >= (int64_t(1) << 31)) return set_last_error(LORA_EINVAL, "W must be < 2^31");
  if (rows >= (int64_t(1) << 31)) return set_last_error(LORA_EINVAL, "batch too large");
  if (rows > 1 && stride < W) return set_last_error(LORA_EINVAL, "stride smaller than windows per row");
  if (rows == 0) return 0;
  if (!count || !end || (capacity > 0 && !starts)) return set_last_error(LORA_EINVAL, "null output");
  const int64_t k = step / p->hop;
  if (W > k && (!power || !power_avg || !index)) return set_last_error(LORA_EINVAL, "null metrics");
  lora::FindArgs a{};
  a.power = power;
  a.power_avg = power_avg;
  a.index = index;
  a.first = first;
  a.starts = starts;
  a.count = count;
  a.end = end;
  a.stride = stride;
  a.capacity = capacity;
  a.n = W - k;
  a.hop = p->hop;
  a.osr = p->osr;
  a.half_step = step / 2;
  a.frame_len = (p->frame_symbols + 2) * step;
  a.last_start = row_len - a.frame_len;
  a.lead_q = (a.frame_len - a.half_step) / p->hop;
  a.lead_r = (int)((a.frame_len - a.half_step) % p->hop);
  a.hop32 = (int)p->hop;  // hop <= step / 2 <= 2^27
  a.k = (int)k;
  a.N = (int)N;
  const int sync = (int)(p->sync & 0xFFu);
  a.sw0 = (sync >> 4) << (p->sf - 4);
  const int sw1 = (sync & 15) << (p->sf - 4);
  a.dsync = (sw1 - a.sw0) & (a.N - 1);
  a.thresh = p->thresh_db;
  lora::DeviceGuard guard(p->device);
  if (guard.err != hipSuccess) return lora::hip_error("find device", guard.err);
  hipLaunchKernelGGL(lora::k_find_frames, dim3((unsigned)rows), dim3(lora::kThreads), 0,
                     static_cast<hipStream_t>(stream), a);
  const hipError_t e = hipGetLastError();
  return e != hipSuccess ? lora::hip_error("k_find_frames", e) : rows;
}

}  // extern "C"
