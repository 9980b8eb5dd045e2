// lora_codec.hip — the payload codec on the device: symbols <-> bytes for whole batches of
// frames, behind lora_decode_batch / lora_encode_batch / lora_decode_chain_batch /
// lora_encode_chain_batch / lora_decode_chain_soft_batch (include/lora_mi355x.h), and the
// self-describing frame's lora_encode_frame_batch / lora_decode_frame_batch /
// lora_decode_frame_soft_batch further down.
//
// The first four are bit-exact integer work, one kernel per call, no workspace, no atomics:
//   k_codec_decode        LoRaDecoder.cpp:8-19 + the CRC check of phy.cpp:241-256
//   k_codec_encode        LoRaEncoder.cpp:8-19 (+ the SX1272 data checksum appended)
//   k_codec_chain_decode  Gray -> diagonal deinterleave -> de-whitening -> nibble decode
//   k_codec_chain_encode  nibble encode -> whitening -> diagonal interleave -> Gray
// and k_soft_chain_decode is k_codec_chain_decode on per-bit LLRs (lora_demod_soft_bits_batch's):
// deinterleave and de-whitening act on the LLRs, the nibble decode is maximum likelihood.
// (LoRaCodes.hpp:176-189, 201-222, 229-371, 376-412; lora_phy_amd/codes.py restates them
// on the host and is the checker in tests/test_gpu_codec.py).
//
// Layout: a frame belongs to a group of G = 2^lg lanes, G the smallest power of two that
// gives every output element of the frame (a byte, or a symbol for the chain encoder) a lane
// of its own, at most 64 (longer frames: the group's lanes stride the frame); 256 / G frames
// per 256-thread workgroup.  The library decoder alone takes frames of any length, and gives
// one of more than 256 bytes a whole workgroup (lg = 8).  Lane l of a group works on elements
// l, l + G, ...: neighbouring lanes touch neighbouring addresses in every global access.
// Per-frame results (checksum, error counts) are reduced across the group's lanes with
// cross-lane moves (plus one LDS step between the four waves of a whole-workgroup frame) and
// written by the group's first lane.
//
// The SX1272 data checksum (LoRaCodes.hpp:92-105) is a CRC-16 (x^16 + x^12 + x^5 + 1) over
// the data in which byte k of m enters 8 (m - 1 - k) shifts before the end, plus a term that
// depends on m alone (an 8-bit LFSR stepped m times).  The CRC is linear over GF(2), so each
// lane multiplies its own byte by x^(8 (m - 1 - k)) mod P - the power from a 256-entry table
// (frames beyond it: square-and-multiply over the constant maps x^(8 2^j)), the product a
// carry-less 8 x 16-bit multiply and a two-step reduction - and the group XORs the terms: no
// lane walks the frame serially.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/lora_mi355x.h"
#include "lora_internal.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxPayload = 255;  // bytes per frame of the encoders and the chain decoder

// ---------------------------------------------------------------------------------
// Constant tables, generated at compile time from the equations
// ---------------------------------------------------------------------------------

// Whitening sequence of the chain (LoRaCodes.hpp:176-189 with bit_ofs = 0): two 64-bit
// registers used alternately, each stepping r -> r >> 8 with the new top byte
// r[39:32] ^ r[31:24] ^ r[23:16] ^ r[7:0]; byte i of the sequence is the low byte of register
// i & 1 before its step.  Two seed classes (RDD 1, and every other RDD); the RDD's mask
// 0xFF >> (4 - RDD) is applied where the byte is used.  A frame holds at most
// ceil(2 * 255 / sf) * sf <= 521 codewords.
constexpr int kWhitenLen = 528;
struct WhitenTab {
  uint8_t v[2][kWhitenLen];
};
constexpr uint64_t whiten_step(uint64_t r) { return (r >> 8) | (((r >> 32) ^ (r >> 24) ^ (r >> 16) ^ r) << 56); }
constexpr WhitenTab make_whiten() {
  WhitenTab t{};
  for (int cls = 0; cls < 2; ++cls) {
    uint64_t r[2] = {cls ? 0x05121100F8ECFEEFull : 0x6572D100E85C2EFFull,
                     cls ? 0xF8ECFEEFEFEFEFEFull : 0xE85C2EFFFFFFFFFFull};
    for (int i = 0; i < kWhitenLen; ++i) {
      t.v[cls][i] = (uint8_t)(r[i & 1] & 0xFF);
      r[i & 1] = whiten_step(r[i & 1]);
    }
  }
  return t;
}
__device__ const WhitenTab kWhiten = make_whiten();

// x -> x * x^8 mod P, P = x^16 + x^12 + x^5 + 1 (one byte step of the checksum's CRC)
constexpr uint16_t crc_shift8(uint16_t x) {
  for (int i = 0; i < 8; ++i) x = (uint16_t)((x & 0x8000) ? ((x << 1) ^ 0x1021) : (x << 1));
  return x;
}
// col[j][i] = x^i * x^(8 * 2^j) mod P: the linear map "shift by 2^j bytes" by columns
// (x has order 32767 modulo P, checked below: 15 levels cover every exponent)
constexpr int kCrcLevels = 15;
constexpr uint32_t kCrcOrder = 32767;
struct CrcPow {
  uint16_t col[kCrcLevels][16];
};
constexpr uint16_t crc_apply(const uint16_t* col, uint16_t x) {
  uint16_t r = 0;
  for (int i = 0; i < 16; ++i)
    if ((x >> i) & 1) r ^= col[i];
  return r;
}
constexpr CrcPow make_crc_pow() {
  CrcPow t{};
  for (int i = 0; i < 16; ++i) t.col[0][i] = crc_shift8((uint16_t)(1u << i));
  for (int j = 1; j < kCrcLevels; ++j)
    for (int i = 0; i < 16; ++i) t.col[j][i] = crc_apply(t.col[j - 1], t.col[j - 1][i]);
  return t;
}
constexpr CrcPow kCrcPowHost = make_crc_pow();
constexpr bool crc_order_ok() {  // shifting by 1 + 2 + ... + 2^14 = 32767 bytes is the identity
  for (int i = 0; i < 16; ++i) {
    uint16_t x = (uint16_t)(1u << i);
    for (int j = 0; j < kCrcLevels; ++j) x = crc_apply(kCrcPowHost.col[j], x);
    if (x != (uint16_t)(1u << i)) return false;
  }
  return true;
}
static_assert(crc_order_ok(), "x^(8 * 32767) must be 1 modulo the CRC polynomial");
__device__ const CrcPow kCrcPow = make_crc_pow();
// x^(8 e) mod P for e < 256: every frame of up to 260 bytes
constexpr int kCrcXLen = 256;
struct CrcX {
  uint16_t v[kCrcXLen];
};
constexpr CrcX make_crc_x() {
  CrcX t{};
  uint16_t x = 1;
  for (int e = 0; e < kCrcXLen; ++e) {
    t.v[e] = x;
    x = crc_shift8(x);
  }
  return t;
}
__device__ const CrcX kCrcX = make_crc_x();

// The checksum's second register: v -> (v << 1 | parity(v & 0xB8)) & 0xFF from 0xFF, once
// per data byte.  The sequence has period 255, so v after m bytes is kCrcV.v[m % 255].
struct CrcV {
  uint8_t v[256];
};
constexpr CrcV make_crc_v() {
  CrcV t{};
  uint8_t v = 0xFF;
  for (int i = 0; i < 256; ++i) {
    t.v[i] = v;
    uint8_t p = v & 0xB8;
    p ^= p >> 4;
    p ^= p >> 2;
    p ^= p >> 1;
    v = (uint8_t)((p & 1) | (v << 1));
  }
  return t;
}
constexpr CrcV kCrcVHost = make_crc_v();
static_assert(kCrcVHost.v[255] == kCrcVHost.v[0], "the checksum's LFSR must repeat after 255 steps");
__device__ const CrcV kCrcV = make_crc_v();

// ---------------------------------------------------------------------------------
// Nibble codes (LoRaCodes.hpp:229-371), as parities of bit masks
// ---------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t par(uint32_t x) { return (uint32_t)__popc(x) & 1u; }

// Hamming 8/4 and its prefixes: bits 4..7 = d0^d1^d2, d1^d2^d3, d0^d1^d3, d0^d2^d3
__device__ __forceinline__ uint32_t enc_h84(uint32_t x) {
  x &= 0xF;
  return x | (par(x & 0x7) << 4) | (par(x & 0xE) << 5) | (par(x & 0xB) << 6) | (par(x & 0xD) << 7);
}
// nibble -> codeword of coding rate 4/(4 + rdd): Hamming 8/4, Hamming 7/4, parity 6/4 (the
// 8/4 code's first two checks), parity 5/4, the bare nibble
__device__ __forceinline__ uint32_t nibble_encode(uint32_t x, int rdd) {
  x &= 0xF;
  if (rdd == 1) return x | (par(x) << 4);
  return enc_h84(x) & (0xFFu >> (4 - rdd));
}

struct Nib {
  uint32_t nib, err, bad;
};
// the four checks of a received Hamming 8/4 codeword
__device__ __forceinline__ uint32_t syndrome(uint32_t b) {
  return par(b & 0x17) | (par(b & 0x2E) << 1) | (par(b & 0x4B) << 2) | (par(b & 0x8D) << 3);
}
// LoRaCodes.hpp:250-281: syndromes 0xD, 0x7, 0xB, 0xE flip data bit 0, 1, 2, 3; a single
// check (1, 2, 4, 8) is a flipped check bit; any other non-zero syndrome is uncorrectable
__device__ __forceinline__ Nib dec_h84(uint32_t b) {
  const uint32_t p = syndrome(b);
  const uint32_t fix = (uint32_t)((0x0810400020000000ull >> (4 * p)) & 0xF);
  return Nib{(b ^ fix) & 0xF, p != 0 ? 1u : 0u, (0x9668u >> p) & 1u};
}
// LoRaCodes.hpp:306-334: three checks; syndromes 5, 7, 3, 6 flip data bit 0, 1, 2, 3
__device__ __forceinline__ Nib dec_h74(uint32_t b) {
  const uint32_t p = syndrome(b) & 7;
  const uint32_t fix = (0x28104000u >> (4 * p)) & 0xF;
  return Nib{(b ^ fix) & 0xF, p != 0 ? 1u : 0u, 0u};
}
// codeword -> nibble and error flag by rdd (Hamming 8/4's 'bad' is an error too)
__device__ __forceinline__ Nib nibble_decode(uint32_t b, int rdd) {
  if (rdd == 4) return dec_h84(b);
  if (rdd == 3) return dec_h74(b);
  if (rdd == 2) return Nib{b & 0xF, par(b & 0x17) | par(b & 0x2E), 0u};
  if (rdd == 1) return Nib{b & 0xF, par(b & 0x1F), 0u};
  return Nib{b & 0xF, 0u, 0u};
}

// LoRaCodes.hpp:212-222
__device__ __forceinline__ uint32_t gray_to_binary16(uint32_t n) {
  n &= 0xFFFF;
  n ^= n >> 8;
  n ^= n >> 4;
  n ^= n >> 2;
  n ^= n >> 1;
  return n;
}

// ---------------------------------------------------------------------------------
// Checksum pieces
// ---------------------------------------------------------------------------------

// x^(8 e) mod P for e < 2^levels <= 2^15: one constant map per set bit of e
__device__ __forceinline__ uint32_t crc_power(uint32_t e, int levels) {
  uint32_t x = 1;
#pragma unroll
  for (int j = 0; j < kCrcLevels; ++j) {
    if (j < levels && ((e >> j) & 1)) {
      uint32_t r = 0;
#pragma unroll
      for (int i = 0; i < 16; ++i) r ^= (0u - ((x >> i) & 1u)) & kCrcPow.col[j][i];
      x = r;
    }
  }
  return x;
}
// byte b of the data, e bytes before its end: b * x^(8 e) mod P.  The product of the byte and
// the power c has degree < 23; its top 7 bits t fold back as t (x^12 + x^5 + 1), whose own
// overflow (t >> 4, 3 bits) folds once more.
__device__ __forceinline__ uint32_t crc_term(uint32_t b, uint32_t e, int levels) {
  const uint32_t c = levels <= 8 ? (uint32_t)kCrcX.v[e] : crc_power(e % kCrcOrder, levels);
  uint32_t prod = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) prod ^= (0u - ((b >> i) & 1u)) & (c << i);
  const uint32_t t = prod >> 16, t2 = t >> 4;
  return (prod ^ t ^ (t << 5) ^ (t << 12) ^ t2 ^ (t2 << 5) ^ (t2 << 12)) & 0xFFFF;
}
// levels for exponents up to emax (0 when there is nothing to shift)
__device__ __forceinline__ int crc_levels(int emax) { return emax > 0 ? min(kCrcLevels, 32 - __clz(emax)) : 0; }

// the checksum of m data bytes from the XOR of their shifted terms (LoRaCodes.hpp:101-104)
__device__ __forceinline__ uint32_t crc_finish(uint32_t terms, int m) {
  return (terms ^ kCrcV.v[m % 255] ^ ((uint32_t)kCrcV.v[(m + 1) % 255] << 8)) & 0xFFFF;
}

// XOR / sum over the lanes of a group of 2^lg <= 64 lanes (groups are aligned in the wave)
__device__ __forceinline__ uint32_t group_xor(uint32_t v, int lg) {
  for (int o = (1 << min(lg, 6)) >> 1; o > 0; o >>= 1) v ^= (uint32_t)__shfl_xor((int)v, o, 64);
  return v;
}
__device__ __forceinline__ uint32_t group_sum(uint32_t v, int lg) {
  for (int o = (1 << min(lg, 6)) >> 1; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
  return v;
}

// two neighbouring symbols of a row (one 4-byte access where the row's alignment allows)
__device__ __forceinline__ void load_pair(const uint16_t* p, uint32_t& s0, uint32_t& s1) {
  if ((reinterpret_cast<uintptr_t>(p) & 3) == 0) {
    const uint32_t w = *reinterpret_cast<const uint32_t*>(p);
    s0 = w & 0xFFFF;
    s1 = w >> 16;
  } else {
    s0 = p[0];
    s1 = p[1];
  }
}
__device__ __forceinline__ void store_pair(uint16_t* p, uint32_t s0, uint32_t s1) {
  if ((reinterpret_cast<uintptr_t>(p) & 3) == 0) {
    *reinterpret_cast<uint32_t*>(p) = s0 | (s1 << 16);
  } else {
    p[0] = (uint16_t)s0;
    p[1] = (uint16_t)s1;
  }
}

// ---------------------------------------------------------------------------------
// Library decoder
// ---------------------------------------------------------------------------------
struct DecArgs {
  const uint16_t* sym;
  int64_t frames, sym_stride, pay_stride;
  int S;   // symbols per frame
  int lg;  // log2 lanes per frame: 0..6, or 8 = a whole workgroup
  uint8_t* pay;
  uint8_t* crc_ok;
  int32_t* err;
  int32_t* bad;
};

__global__ void __launch_bounds__(kBlock) k_codec_decode(DecArgs a) {
  __shared__ uint32_t red[3][kBlock / 64];
  const int tid = threadIdx.x;
  const int G = 1 << a.lg;
  const int l = tid & (G - 1);
  const int64_t f = (int64_t)blockIdx.x * (kBlock >> a.lg) + (tid >> a.lg);
  const bool live = f < a.frames;
  const int n = a.S >> 1;  // bytes; an odd trailing symbol is ignored
  const bool crc = n >= 4;
  const int levels = crc_levels(n - 5);  // data byte d of m = n - 4 shifts m - 1 - d bytes
  // w: the checksum's terms in the low half, the frame's own checksum bytes in the high half
  uint32_t w = 0, ne = 0, nb = 0;
  if (live) {
    const uint16_t* row = a.sym + f * a.sym_stride;
    uint8_t* out = a.pay + f * a.pay_stride;
    for (int k = l; k < n; k += G) {
      uint32_t s0, s1;
      load_pair(row + 2 * k, s0, s1);
      const Nib hi = dec_h84(s0 & 0xFF), lo = dec_h84(s1 & 0xFF);  // the symbols' low byte
      const uint32_t byte = (hi.nib << 4) | lo.nib;
      out[k] = (uint8_t)byte;
      ne += hi.err + lo.err;
      nb += hi.bad + lo.bad;
      if (crc) {
        if (k >= n - 2)
          w ^= byte << (k == n - 2 ? 16 : 24);
        else if (k >= 2)
          w ^= crc_term(byte, (uint32_t)(n - 3 - k), levels);
      }
    }
  }
  w = group_xor(w, a.lg);
  if (a.lg <= 6) {  // at most 512 symbols per group: both counts in one word
    const uint32_t c = group_sum(ne | (nb << 16), a.lg);
    ne = c & 0xFFFF;
    nb = c >> 16;
  } else {  // a whole-workgroup frame: the four waves' results through LDS
    ne = group_sum(ne, a.lg);
    nb = group_sum(nb, a.lg);
    if ((tid & 63) == 0) {
      red[0][tid >> 6] = w;
      red[1][tid >> 6] = ne;
      red[2][tid >> 6] = nb;
    }
    __syncthreads();
    w = red[0][0] ^ red[0][1] ^ red[0][2] ^ red[0][3];
    ne = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    nb = red[2][0] + red[2][1] + red[2][2] + red[2][3];
  }
  if (live && l == 0) {
    if (a.crc_ok) a.crc_ok[f] = (crc && crc_finish(w & 0xFFFF, n - 4) == (w >> 16)) ? 1 : 0;
    if (a.err) a.err[f] = (int32_t)ne;
    if (a.bad) a.bad[f] = (int32_t)nb;
  }
}

// ---------------------------------------------------------------------------------
// Library encoder
// ---------------------------------------------------------------------------------
struct EncArgs {
  const uint8_t* pay;
  int64_t frames, pay_stride, sym_stride;
  int nbytes, append_crc;
  int lg;  // 0..6
  uint16_t* sym;
};

__global__ void __launch_bounds__(kBlock) k_codec_encode(EncArgs a) {
  const int tid = threadIdx.x;
  const int G = 1 << a.lg;
  const int l = tid & (G - 1);
  const int64_t f = (int64_t)blockIdx.x * (kBlock >> a.lg) + (tid >> a.lg);
  const bool live = f < a.frames;
  const int n = a.nbytes;
  const int levels = a.append_crc ? crc_levels(n - 3) : 0;  // data = bytes[2:], byte k shifts n - 1 - k
  uint32_t w = 0;
  uint16_t* row = a.sym + (live ? f : 0) * a.sym_stride;
  if (live) {
    const uint8_t* in = a.pay + f * a.pay_stride;
    for (int k = l; k < n; k += G) {
      const uint32_t b = in[k];
      store_pair(row + 2 * k, enc_h84(b >> 4), enc_h84(b & 0xF));  // high nibble first
      if (a.append_crc && k >= 2) w ^= crc_term(b, (uint32_t)(n - 1 - k), levels);
    }
  }
  if (!a.append_crc) return;
  w = group_xor(w, a.lg);
  if (live && l == 0) {  // the checksum, low byte first, as two more encoded bytes
    const uint32_t c = crc_finish(w, n > 2 ? n - 2 : 0);
    store_pair(row + 2 * n, enc_h84((c >> 4) & 0xF), enc_h84(c & 0xF));
    store_pair(row + 2 * n + 2, enc_h84(c >> 12), enc_h84((c >> 8) & 0xF));
  }
}

// ---------------------------------------------------------------------------------
// The coding chain
// ---------------------------------------------------------------------------------
struct ChainArgs {
  int sf, rdd, nbytes;
  int lg;    // 0..6
  int nsym;  // decoder: symbols the payload's blocks span; encoder: symbols per frame
  int ncw;   // encoder: codewords per frame (a multiple of sf)
  int64_t frames, sym_stride, pay_stride;
  const uint16_t* sym_in;
  uint16_t* sym_out;
  const uint8_t* pay_in;
  uint8_t* pay_out;
  int32_t* err;
};

// LDS of a workgroup's frames.  The decoder stages nsym <= 8 ceil(2 nbytes / 6) binary symbols
// per frame, nbytes <= G below 64 lanes and <= 255 with 64: (256 / G) * nsym <= 2752.  The
// encoder stages ncw <= 3 nsym codewords, nsym <= G below 64 lanes and ncw <= 521 with 64.
// (the host checks both products before it launches)
constexpr int kChainDecLds = 2816;
constexpr int kChainEncLds = 2304;

__global__ void __launch_bounds__(kBlock) k_codec_chain_decode(ChainArgs a) {
  __shared__ uint16_t sh[kChainDecLds];
  const int tid = threadIdx.x;
  const int G = 1 << a.lg;
  const int l = tid & (G - 1);
  const int64_t f = (int64_t)blockIdx.x * (kBlock >> a.lg) + (tid >> a.lg);
  const bool live = f < a.frames;
  const int nbits = 4 + a.rdd;
  uint16_t* my = sh + (tid >> a.lg) * a.nsym;
  if (live) {  // the frame's symbols, Gray -> binary (LoRaCodes.hpp:212-222)
    const uint16_t* row = a.sym_in + f * a.sym_stride;
    for (int i = l; i < a.nsym; i += G) my[i] = (uint16_t)gray_to_binary16(row[i]);
  }
  __syncthreads();
  uint32_t ne = 0;
  if (live) {
    const uint8_t* wh = kWhiten.v[a.rdd == 1 ? 1 : 0];
    const uint32_t mask = 0xFFu >> (4 - a.rdd);
    uint8_t* out = a.pay_out + f * a.pay_stride;
    for (int k = l; k < a.nbytes; k += G) {
      uint32_t byte = 0;
      for (int h = 0; h < 2; ++h) {
        // codeword c = row `dst` of block `blk`: its bit `bit` is bit (dst - bit) mod sf of
        // the block's symbol `bit` (LoRaCodes.hpp:396-412)
        const int c = 2 * k + h;
        const int blk = c / a.sf;
        const int dst = c - blk * a.sf;
        const uint16_t* s = my + blk * nbits;
        uint32_t cw = 0;
        for (int bit = 0; bit < nbits; ++bit) {
          const int ci = (dst + 2 * a.sf - bit) % a.sf;
          cw |= (((uint32_t)s[bit] >> ci) & 1u) << bit;
        }
        cw ^= wh[c] & mask;
        const Nib d = nibble_decode(cw, a.rdd);
        byte = (byte << 4) | d.nib;
        ne += d.err;
      }
      out[k] = (uint8_t)byte;
    }
  }
  ne = group_sum(ne, a.lg);
  if (live && l == 0 && a.err) a.err[f] = (int32_t)ne;
}

// The chain decoder on soft bits: each codeword's 4 + rdd LLRs are gathered through the
// deinterleave map straight from global memory (every LLR of the frame's blocks is read by
// exactly one lane, so nothing is staged), their signs follow the whitening sequence, and the
// nibble is the candidate with the largest correlation.  fp32 additions only, in bit order.
// One instance per RDD: the 16 candidate codewords and the bit count are constants.
struct SoftArgs {
  ChainArgs c;
  const float* llr;  // [frames][c.sym_stride][c.sf]
};
template <int RDD>
__global__ void __launch_bounds__(kBlock) k_soft_chain_decode(SoftArgs sa) {
  const ChainArgs& a = sa.c;
  const float* __restrict__ llr = sa.llr;
  const int tid = threadIdx.x;
  const int G = 1 << a.lg;
  const int l = tid & (G - 1);
  const int64_t f = (int64_t)blockIdx.x * (kBlock >> a.lg) + (tid >> a.lg);
  const bool live = f < a.frames;
  constexpr int nbits = 4 + RDD;
  uint32_t nc = 0;
  if (live) {
    const uint8_t* wh = kWhiten.v[RDD == 1 ? 1 : 0];
    const uint32_t mask = 0xFFu >> (4 - RDD);
    const float* row = llr + f * a.sym_stride * a.sf;
    uint8_t* out = a.pay_out + f * a.pay_stride;
    for (int k = l; k < a.nbytes; k += G) {
      uint32_t byte = 0;
      for (int h = 0; h < 2; ++h) {
        // codeword c = row `dst` of block `blk`: its bit `bit` is bit (dst - bit) mod sf of
        // the block's symbol `bit` (LoRaCodes.hpp:396-412)
        const int c = 2 * k + h;
        const int blk = c / a.sf;
        const int dst = c - blk * a.sf;
        const float* s = row + (size_t)blk * nbits * a.sf;
        const uint32_t w = wh[c] & mask;
        float L[nbits];
        uint32_t hard = 0;
#pragma unroll
        for (int bit = 0; bit < nbits; ++bit) {
          const int ci = (dst + 2 * a.sf - bit) % a.sf;
          float v = s[bit * a.sf + ci];
          if ((w >> bit) & 1u) v = -v;
          if (v > 0.0f) hard |= 1u << bit;
          L[bit] = v;
        }
        float best = -__builtin_inff();
        uint32_t nib = 0;
#pragma unroll
        for (uint32_t x = 0; x < 16; ++x) {
          const uint32_t e = nibble_encode(x, RDD);
          float m = 0.0f;
#pragma unroll
          for (int bit = 0; bit < nbits; ++bit) m = m + (((e >> bit) & 1u) ? L[bit] : -L[bit]);
          if (m > best) {
            best = m;
            nib = x;
          }
        }
        byte = (byte << 4) | nib;
        nc += nibble_encode(nib, RDD) != hard ? 1u : 0u;
      }
      out[k] = (uint8_t)byte;
    }
  }
  nc = group_sum(nc, a.lg);
  if (live && l == 0 && a.err) a.err[f] = (int32_t)nc;
}

__global__ void __launch_bounds__(kBlock) k_codec_chain_encode(ChainArgs a) {
  __shared__ uint8_t sh[kChainEncLds];
  const int tid = threadIdx.x;
  const int G = 1 << a.lg;
  const int l = tid & (G - 1);
  const int64_t f = (int64_t)blockIdx.x * (kBlock >> a.lg) + (tid >> a.lg);
  const bool live = f < a.frames;
  const int nbits = 4 + a.rdd;
  uint8_t* my = sh + (tid >> a.lg) * a.ncw;
  if (live) {  // whitened codewords; the padding is zero codewords, whitened too
    const uint8_t* wh = kWhiten.v[a.rdd == 1 ? 1 : 0];
    const uint32_t mask = 0xFFu >> (4 - a.rdd);
    const uint8_t* in = a.pay_in + f * a.pay_stride;
    for (int c = l; c < a.ncw; c += G) {
      uint32_t cw = 0;
      if (c < 2 * a.nbytes) {
        const uint32_t b = in[c >> 1];
        cw = nibble_encode((c & 1) ? b : b >> 4, a.rdd);  // high nibble first
      }
      my[c] = (uint8_t)(cw ^ (wh[c] & mask));
    }
  }
  __syncthreads();
  if (live) {
    uint16_t* row = a.sym_out + f * a.sym_stride;
    for (int s = l; s < a.nsym; s += G) {
      // symbol `bit` of block `blk`: its bit c is bit `bit` of the block's codeword
      // (c + bit) mod sf (LoRaCodes.hpp:376-394); then binary -> Gray
      const int blk = s / nbits;
      const int bit = s - blk * nbits;
      const uint8_t* cw = my + blk * a.sf;
      uint32_t v = 0;
      for (int c = 0; c < a.sf; ++c) v |= (((uint32_t)cw[(c + bit) % a.sf] >> bit) & 1u) << c;
      row[s] = (uint16_t)(v ^ (v >> 1));
    }
  }
}

// ---------------------------------------------------------------------------------
// Self-describing frames (the definition is in include/lora_mi355x.h)
// ---------------------------------------------------------------------------------
// Nothing is staged: a lane builds each symbol it writes (encoder) or each byte it writes
// (decoder) from the codewords it needs, which it computes from the frame's bytes or symbols
// in global memory - a frame is a few hundred bytes that stay in the cache - so the kernels
// need no LDS and no barrier.  The header is eight symbols: every lane of a frame's group
// decodes it for itself.

// the remaining blocks' whitening starts sf - 7 bytes into the sequence: the last byte used is
// ceil(K / sf) * sf + sf - 8 with K = 2 * 257 - (sf - 7) codewords
constexpr bool frame_whiten_fits() {
  for (int sf = 7; sf <= 12; ++sf)
    if ((2 * (kMaxPayload + 2) - (sf - 7) + sf - 1) / sf * sf + (sf - 7) > kWhitenLen) return false;
  return true;
}
static_assert(frame_whiten_fits(), "the whitening table must cover a frame of 255 bytes and its CRC");

__host__ __device__ inline int frame_nsym(int sf, int rdd, int n, int crc) {
  const int nd = 2 * (n + 2 * crc);
  const int k = nd > sf - 7 ? nd - (sf - 7) : 0;
  return 8 + (k + sf - 1) / sf * (4 + rdd);
}

// headerChecksum (LoRaCodes.hpp:43-67) of h0 | h1 << 8: each of its five bits is a parity
__device__ __forceinline__ uint32_t header_checksum(uint32_t w) {
  return (par(w & 0x0F0) << 4) | (par(w & 0x18E) << 3) | (par(w & 0xA49) << 2) | (par(w & 0x725) << 1) |
         par(w & 0xF12);
}

struct FrameEncArgs {
  int sf, rdd, crc, max_bytes;
  int lg;    // 0..6
  int cols;  // symbols written per row: those of a frame of max_bytes
  int64_t frames, pay_stride, sym_stride;
  const uint8_t* pay;
  const int32_t* nbytes;  // NULL: max_bytes for every frame
  uint16_t* sym;
  int32_t* nsym;
};

// data nibble i of a frame of n payload bytes and checksum c (its low byte first), high nibble
// of a byte first
__device__ __forceinline__ uint32_t frame_nibble(const uint8_t* in, int n, uint32_t c, int i) {
  const int k = i >> 1;
  const uint32_t b = k < n ? in[k] : (k == n ? c & 0xFF : c >> 8);
  return (i & 1) ? b & 0xF : b >> 4;
}

__global__ void __launch_bounds__(kBlock) k_frame_encode(FrameEncArgs a) {
  const int tid = threadIdx.x;
  const int G = 1 << a.lg;
  const int l = tid & (G - 1);
  const int64_t f = (int64_t)blockIdx.x * (kBlock >> a.lg) + (tid >> a.lg);
  const bool live = f < a.frames;
  const uint8_t* in = a.pay + (live ? f : 0) * a.pay_stride;
  int n = 0;
  if (live) n = a.nbytes ? min(max(a.nbytes[f], 0), a.max_bytes) : a.max_bytes;
  uint32_t w = 0;
  if (a.crc) {  // the checksum of all n bytes: byte k shifts n - 1 - k bytes (< 256: the table)
    const int levels = crc_levels(n - 1);
    for (int k = l; k < n; k += G) w ^= crc_term(in[k], (uint32_t)(n - 1 - k), levels);
    w = crc_finish(group_xor(w, a.lg), n);
  }
  if (!live) return;
  const int sf = a.sf, rdd = a.rdd, nbits = 4 + rdd, nh = sf - 7;
  const int nd = 2 * (n + 2 * a.crc);
  const int ns = frame_nsym(sf, rdd, n, a.crc);
  const uint32_t h1 = (uint32_t)(rdd << 1) | (uint32_t)a.crc;
  const uint32_t h2 = header_checksum((uint32_t)n | (h1 << 8));
  // the header's nibbles, four bits each from bit 0
  const uint32_t hw = ((uint32_t)n >> 4) | (((uint32_t)n & 15) << 4) | (h1 << 8) | ((h2 >> 4) << 12) | ((h2 & 15) << 16);
  const uint8_t* wh = kWhiten.v[rdd == 1 ? 1 : 0];
  const uint32_t mask = 0xFFu >> (4 - rdd);
  uint16_t* row = a.sym + f * a.sym_stride;
  for (int s = l; s < a.cols; s += G) {
    uint32_t v = 0;
    if (s < 8) {
      // symbol `s` of block 0: its bit c is bit s of the block's codeword (c + s) mod (sf - 2)
      // (LoRaCodes.hpp:376-394 at PPM sf - 2); Gray, then two bins per value step
      const int ppm = sf - 2;
      for (int c = 0; c < ppm; ++c) {
        const int j = (c + s) % ppm;
        uint32_t cw;
        if (j < 5) {
          cw = enc_h84((hw >> (4 * j)) & 15);
        } else {
          cw = j - 5 < nd ? enc_h84(frame_nibble(in, n, w, j - 5)) : 0u;
          cw ^= kWhiten.v[0][j - 5];
        }
        v |= ((cw >> s) & 1u) << c;
      }
      v = (v ^ (v >> 1)) << 2;
    } else if (s < ns) {
      const int blk = (s - 8) / nbits;
      const int bit = (s - 8) - blk * nbits;
      for (int c = 0; c < sf; ++c) {
        const int j = blk * sf + (c + bit) % sf;  // codeword of the remaining blocks
        uint32_t cw = nh + j < nd ? nibble_encode(frame_nibble(in, n, w, nh + j), rdd) : 0u;
        cw ^= wh[nh + j] & mask;
        v |= ((cw >> bit) & 1u) << c;
      }
      v ^= v >> 1;
    }
    row[s] = (uint16_t)v;
  }
  if (l == 0 && a.nsym) a.nsym[f] = ns;
}

struct FrameDecArgs {
  int sf, max_bytes;
  int lg;    // 0..6
  int cols;  // symbols per row
  int64_t frames, sym_stride, pay_stride;
  const uint16_t* sym;
  const int32_t* avail;  // NULL: cols for every frame
  int32_t *status, *nbytes, *rdd, *has_crc, *nsym, *errors;
  uint8_t* pay;  // NULL: header-only mode
};

// codeword j of block 0 from its eight binary symbols: bit `bit` is bit (j - bit) mod ppm of
// symbol `bit` (LoRaCodes.hpp:396-412 at PPM sf - 2)
__device__ __forceinline__ uint32_t block0_codeword(const uint32_t (&hs)[8], int ppm, int j) {
  uint32_t cw = 0;
#pragma unroll
  for (int bit = 0; bit < 8; ++bit) cw |= ((hs[bit] >> ((j + 2 * ppm - bit) % ppm)) & 1u) << bit;
  return cw;
}

__global__ void __launch_bounds__(kBlock) k_frame_decode(FrameDecArgs a) {
  const int tid = threadIdx.x;
  const int G = 1 << a.lg;
  const int l = tid & (G - 1);
  const int64_t f = (int64_t)blockIdx.x * (kBlock >> a.lg) + (tid >> a.lg);
  const bool live = f < a.frames;
  const int sf = a.sf, nh = sf - 7;
  const uint16_t* row = a.sym + (live ? f : 0) * a.sym_stride;
  int av = 0;
  if (live) av = a.avail ? min(max(a.avail[f], 0), a.cols) : a.cols;
  int status = LORA_FRAME_SHORT, n = 0, rdd = 0, crc = 0, ns = 0;
  uint32_t herr = 0;
  uint32_t hs[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (av >= 8) {
    // the header's symbols: to the nearest multiple of four bins, Gray -> binary
#pragma unroll
    for (int i = 0; i < 8; ++i) hs[i] = gray_to_binary16((((uint32_t)row[i] + 2u) >> 2) & ((1u << (sf - 2)) - 1u));
    uint32_t hw = 0, hbad = 0;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const Nib d = dec_h84(block0_codeword(hs, sf - 2, j));
      hw |= d.nib << (4 * j);
      herr += d.err;  // set for a bad codeword too
      hbad |= d.bad;
    }
    const uint32_t h0 = ((hw & 15) << 4) | ((hw >> 4) & 15), h1 = (hw >> 8) & 15;
    const uint32_t h2 = (((hw >> 12) & 15) << 4) | ((hw >> 16) & 15);
    if (hbad || h2 > 31 || header_checksum(h0 | (h1 << 8)) != h2 || (h1 >> 1) > 4) {
      status = LORA_FRAME_HEADER;
      herr = 0;
    } else {
      status = LORA_FRAME_OK;
      n = (int)h0;
      rdd = (int)(h1 >> 1);
      crc = (int)(h1 & 1);
      ns = frame_nsym(sf, rdd, n, crc);
    }
  }
  uint32_t w = 0, ne = 0;  // w as in k_codec_decode: checksum terms low, received checksum high
  if (a.pay) {
    const bool whole = status == LORA_FRAME_OK && ns <= av && n <= a.max_bytes;
    if (status == LORA_FRAME_OK && !whole) status = LORA_FRAME_SHORT;
    if (live) {
      const int nbits = 4 + rdd;
      const int nd = whole ? n + 2 * crc : 0;  // data bytes to decode
      const int levels = crc_levels(n - 1);
      const uint8_t* wh = kWhiten.v[rdd == 1 ? 1 : 0];
      const uint32_t mask = 0xFFu >> (4 - rdd);
      uint8_t* out = a.pay + f * a.pay_stride;
      for (int k = l; k < max(nd, a.max_bytes); k += G) {
        if (k >= nd) {
          out[k] = 0;
          continue;
        }
        uint32_t byte = 0;
        for (int h = 0; h < 2; ++h) {
          const int i = 2 * k + h;  // data nibble
          Nib d;
          if (i < nh) {
            d = dec_h84(block0_codeword(hs, sf - 2, 5 + i) ^ kWhiten.v[0][i]);
          } else {
            // codeword c = row `dst` of block `blk` of the remaining blocks, as in
            // k_codec_chain_decode
            const int c = i - nh;
            const int blk = c / sf;
            const int dst = c - blk * sf;
            const uint16_t* s = row + 8 + blk * nbits;
            uint32_t cw = 0;
            for (int bit = 0; bit < nbits; ++bit)
              cw |= ((gray_to_binary16(s[bit]) >> ((dst + 2 * sf - bit) % sf)) & 1u) << bit;
            d = nibble_decode(cw ^ (wh[i] & mask), rdd);
          }
          byte = (byte << 4) | d.nib;
          ne += d.err;
        }
        if (k < n) {
          out[k] = (uint8_t)byte;
          if (crc) w ^= crc_term(byte, (uint32_t)(n - 1 - k), levels);
        } else {
          w ^= byte << (k == n ? 16 : 24);
          if (k < a.max_bytes) out[k] = 0;
        }
      }
    }
    w = group_xor(w, a.lg);
    ne = group_sum(ne, a.lg);
    if (whole && crc && crc_finish(w & 0xFFFF, n) != (w >> 16)) status = LORA_FRAME_CRC;
  }
  if (live && l == 0) {
    if (a.status) a.status[f] = status;
    if (a.nbytes) a.nbytes[f] = n;
    if (a.rdd) a.rdd[f] = rdd;
    if (a.has_crc) a.has_crc[f] = crc;
    if (a.nsym) a.nsym[f] = ns;
    if (a.errors) a.errors[f] = (int32_t)(herr + ne);
  }
}

// k_frame_decode on soft bits (lora_decode_frame_soft_batch): the same layout - a group of lanes
// per frame, nothing staged, every lane decodes the header for itself - with every codeword's
// LLRs gathered through the deinterleave maps straight from global memory, as
// k_soft_chain_decode gathers them.
//
// The coding rate comes from the header, so it differs between the frames of a wave.  One
// decoder serves every rate: a codeword is always eight LLRs, those beyond its 4 + rdd bits +0.0
// (adding +-0 to a metric that starts at +0.0 leaves every bit of it), and the 16 candidates
// are selected by rdd.  Signs are flipped with XOR on the sign bit - what fp32 negation is -
// so neither the whitening nor the candidates' bits cost a lane mask.  (Five inlined per-RDD
// loops behind a switch, with selects for the signs, spilled 80 scalar registers.)  One
// instance per SF: the row pitch and the two interleaver widths are constants.
struct FrameSoftArgs {
  int max_bytes, max_flips;
  int lg;    // 0..6
  int cols;  // columns per row
  int64_t frames, sym_stride, pay_stride;
  const float* llr;      // [frames][sym_stride][sf]
  const int32_t* avail;  // NULL: cols for every frame
  int32_t *status, *nbytes, *rdd, *has_crc, *nsym, *corrected, *hdr_flips;
  uint8_t* pay;  // NULL: header-only mode
};

// Codeword j of a block of width md (sf - 2 or sf) whose first row is s: bit `bit` < 4 + rdd is
// column (j - bit) mod md of row `bit`, its sign flipped where the whitening byte wb has the bit
// set.  Returns the nibble whose codeword at rate 4 / (4 + rdd) has the largest metric
// (k_soft_chain_decode's: fp32 additions in bit order from +0.0, scanned upward with a strict
// '>'), and in `diff` that codeword XOR the hard word (bit = LLR > 0).
template <int SF>
__device__ __forceinline__ uint32_t soft_codeword(const float* __restrict__ s, int md, int j, uint32_t wb, int rdd,
                                                  uint32_t& diff) {
  const int nbits = 4 + rdd;
  float L[8];
  uint32_t hard = 0;
#pragma unroll
  for (int bit = 0; bit < 8; ++bit) {
    // a bit beyond the codeword reads the codeword's last row (which is there) and is zeroed
    const int rb = bit < 4 ? bit : min(bit, nbits - 1);
    int col = j - rb;  // (j - rb) mod md without a division: j - rb >= -7 >= -2 md + 3
    col += col < 0 ? md : 0;
    col += col < 0 ? md : 0;
    uint32_t u = __float_as_uint(s[rb * SF + col]);
    u ^= ((wb >> bit) & 1u) << 31;
    if (bit >= 4) u &= (uint32_t)((bit - nbits) >> 31);  // all ones where bit < nbits
    const float v = __uint_as_float(u);
    hard |= (v > 0.0f ? 1u : 0u) << bit;
    L[bit] = v;
  }
  const bool parity = rdd == 1;  // the one rate whose code is not a prefix of Hamming 8/4
  const uint32_t emask = 0xFFu >> (4 - rdd);
  float best = -__builtin_inff();
  uint32_t nib = 0, chosen = 0;
#pragma unroll
  for (uint32_t x = 0; x < 16; ++x) {
    const uint32_t e = parity ? nibble_encode(x, 1) : enc_h84(x) & emask;
    float m = 0.0f;
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) m = m + __uint_as_float(__float_as_uint(L[bit]) ^ (((~e >> bit) & 1u) << 31));
    if (m > best) {
      best = m;
      nib = x;
      chosen = e;
    }
  }
  diff = chosen ^ hard;
  return nib;
}

template <int SF>
__global__ void __launch_bounds__(kBlock) k_frame_decode_soft(FrameSoftArgs a) {
  const int tid = threadIdx.x;
  const int G = 1 << a.lg;
  const int l = tid & (G - 1);
  const int64_t f = (int64_t)blockIdx.x * (kBlock >> a.lg) + (tid >> a.lg);
  const bool live = f < a.frames;
  constexpr int sf = SF;
  const float* __restrict__ row = a.llr + (live ? f : 0) * a.sym_stride * sf;
  int av = 0;
  if (live) av = a.avail ? min(max(a.avail[f], 0), a.cols) : a.cols;
  int status = LORA_FRAME_SHORT, n = 0, rdd = 0, crc = 0, ns = 0;
  uint32_t hcorr = 0, flips = 0;
  if (av >= 8) {
    uint32_t hw = 0;
#pragma unroll 1
    for (int j = 0; j < 5; ++j) {
      uint32_t diff;
      hw |= soft_codeword<SF>(row, SF - 2, j, 0u, 4, diff) << (4 * j);
      hcorr += diff != 0 ? 1u : 0u;
      flips += (uint32_t)__popc(diff);
    }
    const uint32_t h0 = ((hw & 15) << 4) | ((hw >> 4) & 15), h1 = (hw >> 8) & 15;
    const uint32_t h2 = (((hw >> 12) & 15) << 4) | ((hw >> 16) & 15);
    if (h2 > 31 || header_checksum(h0 | (h1 << 8)) != h2 || (h1 >> 1) > 4 || flips > (uint32_t)a.max_flips) {
      status = LORA_FRAME_HEADER;
      hcorr = 0;
    } else {
      status = LORA_FRAME_OK;
      n = (int)h0;
      rdd = (int)(h1 >> 1);
      crc = (int)(h1 & 1);
      ns = frame_nsym(sf, rdd, n, crc);
    }
  }
  uint32_t w = 0, nc = 0;  // w as in k_codec_decode: checksum terms low, received checksum high
  if (a.pay) {
    const bool whole = status == LORA_FRAME_OK && ns <= av && n <= a.max_bytes;
    if (status == LORA_FRAME_OK && !whole) status = LORA_FRAME_SHORT;
    if (live) {
      const int nbits = 4 + rdd, nh = SF - 7;
      const int nd = whole ? n + 2 * crc : 0;  // data bytes to decode
      const int levels = crc_levels(n - 1);
      const uint8_t* wh = kWhiten.v[rdd == 1 ? 1 : 0];
      const uint32_t mask = 0xFFu >> (4 - rdd);
      uint8_t* out = a.pay + f * a.pay_stride;
      for (int k = l; k < max(nd, a.max_bytes); k += G) {
        if (k >= nd) {
          out[k] = 0;
          continue;
        }
        uint32_t byte = 0;
        for (int h = 0; h < 2; ++h) {
          const int i = 2 * k + h;  // data nibble
          // nibbles below nh: codeword 5 + i of block 0, Hamming 8/4; the others: codeword c =
          // row `dst` of block `blk` of the remaining blocks, as in k_soft_chain_decode
          const bool first = i < nh;
          const int c = first ? 0 : i - nh;
          const int blk = c / SF;
          const int dst = c - blk * SF;
          const float* s = first ? row : row + (size_t)(8 + blk * nbits) * SF;
          const uint32_t wb = first ? kWhiten.v[0][i] : wh[i] & mask;
          uint32_t diff;
          const uint32_t nib = soft_codeword<SF>(s, first ? SF - 2 : SF, first ? 5 + i : dst, wb, first ? 4 : rdd, diff);
          byte = (byte << 4) | nib;
          nc += diff != 0 ? 1u : 0u;
        }
        if (k < n) {
          out[k] = (uint8_t)byte;
          if (crc) w ^= crc_term(byte, (uint32_t)(n - 1 - k), levels);
        } else {
          w ^= byte << (k == n ? 16 : 24);
          if (k < a.max_bytes) out[k] = 0;
        }
      }
    }
    w = group_xor(w, a.lg);
    nc = group_sum(nc, a.lg);
    if (whole && crc && crc_finish(w & 0xFFFF, n) != (w >> 16)) status = LORA_FRAME_CRC;
  }
  if (live && l == 0) {
    if (a.status) a.status[f] = status;
    if (a.nbytes) a.nbytes[f] = n;
    if (a.rdd) a.rdd[f] = rdd;
    if (a.has_crc) a.has_crc[f] = crc;
    if (a.nsym) a.nsym[f] = ns;
    if (a.corrected) a.corrected[f] = (int32_t)(hcorr + nc);
    if (a.hdr_flips) a.hdr_flips[f] = (int32_t)flips;
  }
}

// ---------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------
using lora::set_last_error;

// log2 of the lanes a frame of `work` elements gets: the smallest power of two >= work, <= 64
int group_lg(int64_t work) {
  int lg = 0;
  while (lg < 6 && (int64_t(1) << lg) < work) ++lg;
  return lg;
}

bool chain_params_ok(int sf, int rdd, int64_t nbytes) {
  return sf >= 6 && sf <= 12 && rdd >= 0 && rdd <= 4 && nbytes >= 0 && nbytes <= kMaxPayload;
}
int64_t chain_blocks(int sf, int64_t nbytes) { return (2 * nbytes + sf - 1) / sf; }

// one kernel on `stream` of `device`, 256 >> lg frames per workgroup
template <class K, class A>
int64_t launch_frames(K kernel, const A& a, int64_t frames, int lg, int device, void* stream, int64_t ret) {
  const int64_t blocks = (frames + (kBlock >> lg) - 1) / (kBlock >> lg);
  if (blocks >= (int64_t(1) << 31)) return set_last_error(LORA_EINVAL, "batch too large");
  lora::DeviceGuard guard(device);
  if (guard.err != hipSuccess) return lora::hip_error("codec device", guard.err);
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream), a);
  const hipError_t e = hipGetLastError();
  return e != hipSuccess ? lora::hip_error("codec launch", e) : ret;
}

}  // namespace

int64_t lora_chain_symbols(int sf, int rdd, int64_t nbytes) {
  if (!chain_params_ok(sf, rdd, nbytes))
    return set_last_error(LORA_EINVAL, "sf must be in 6..12, rdd in 0..4, nbytes in 0..255");
  return chain_blocks(sf, nbytes) * (4 + rdd);
}

int64_t lora_decode_batch(const uint16_t* symbols, int64_t frames, int64_t sym_count, int64_t sym_stride,
                          uint8_t* payload, int64_t payload_stride, uint8_t* crc_ok, int32_t* err_count,
                          int32_t* bad_count, int device, void* stream) {
  if (frames < 0 || sym_count < 0 || sym_count >= (int64_t(1) << 31))
    return set_last_error(LORA_EINVAL, "bad frames / sym_count");
  const int64_t n = sym_count / 2;
  if (sym_stride < sym_count) return set_last_error(LORA_EINVAL, "sym_stride smaller than sym_count");
  if (payload_stride < n) return set_last_error(LORA_EINVAL, "payload_stride smaller than the bytes per frame");
  if (frames == 0) return n;
  if (n > 0 && (!symbols || !payload)) return set_last_error(LORA_EINVAL, "null buffer");
  if (n == 0 && !crc_ok && !err_count && !bad_count) return n;  // nothing to write
  DecArgs a;
  a.sym = symbols;
  a.frames = frames;
  a.sym_stride = sym_stride;
  a.pay_stride = payload_stride;
  a.S = (int)sym_count;
  a.lg = n > kBlock ? 8 : group_lg(n);
  a.pay = payload;
  a.crc_ok = crc_ok;
  a.err = err_count;
  a.bad = bad_count;
  return launch_frames(k_codec_decode, a, frames, a.lg, device, stream, n);
}

int64_t lora_encode_batch(const uint8_t* payload, int64_t frames, int64_t nbytes, int64_t payload_stride,
                          int append_crc, uint16_t* symbols, int64_t sym_stride, int device, void* stream) {
  if (frames < 0 || nbytes < 0) return set_last_error(LORA_EINVAL, "bad frames / nbytes");
  if (nbytes > kMaxPayload) return set_last_error(LORA_EINVAL, "nbytes must be <= 255");
  const int64_t nsym = 2 * (nbytes + (append_crc ? 2 : 0));
  if (payload_stride < nbytes) return set_last_error(LORA_EINVAL, "payload_stride smaller than nbytes");
  if (sym_stride < nsym) return set_last_error(LORA_EINVAL, "sym_stride smaller than the symbols per frame");
  if (frames == 0 || nsym == 0) return nsym;
  if (!symbols || (nbytes > 0 && !payload)) return set_last_error(LORA_EINVAL, "null buffer");
  EncArgs a;
  a.pay = payload;
  a.frames = frames;
  a.pay_stride = payload_stride;
  a.sym_stride = sym_stride;
  a.nbytes = (int)nbytes;
  a.append_crc = append_crc ? 1 : 0;
  a.lg = group_lg(nbytes);
  a.sym = symbols;
  return launch_frames(k_codec_encode, a, frames, a.lg, device, stream, nsym);
}

int64_t lora_decode_chain_batch(int sf, int rdd, const uint16_t* symbols, int64_t frames, int64_t sym_count,
                                int64_t sym_stride, int64_t nbytes, uint8_t* payload, int64_t payload_stride,
                                int32_t* err_count, int device, void* stream) {
  if (!chain_params_ok(sf, rdd, nbytes))
    return set_last_error(LORA_EINVAL, "sf must be in 6..12, rdd in 0..4, nbytes in 0..255");
  if (frames < 0 || sym_count < 0) return set_last_error(LORA_EINVAL, "bad frames / sym_count");
  if (sym_stride < sym_count) return set_last_error(LORA_EINVAL, "sym_stride smaller than sym_count");
  if (payload_stride < nbytes) return set_last_error(LORA_EINVAL, "payload_stride smaller than nbytes");
  // whole blocks of 4 + rdd symbols give sf codewords each; trailing symbols are ignored
  if (2 * nbytes > sym_count / (4 + rdd) * sf)
    return set_last_error(LORA_ERANGE, "nbytes needs more codewords than sym_count yields");
  if (frames == 0) return nbytes;
  if (nbytes > 0 && (!symbols || !payload)) return set_last_error(LORA_EINVAL, "null buffer");
  if (nbytes == 0 && !err_count) return nbytes;  // nothing to write
  ChainArgs a{};
  a.sf = sf;
  a.rdd = rdd;
  a.nbytes = (int)nbytes;
  a.lg = group_lg(nbytes);
  a.nsym = (int)(chain_blocks(sf, nbytes) * (4 + rdd));
  a.frames = frames;
  a.sym_stride = sym_stride;
  a.pay_stride = payload_stride;
  a.sym_in = symbols;
  a.pay_out = payload;
  a.err = err_count;
  if ((int64_t)(kBlock >> a.lg) * a.nsym > kChainDecLds) return set_last_error(LORA_EINVAL, "frame too long");
  return launch_frames(k_codec_chain_decode, a, frames, a.lg, device, stream, nbytes);
}

int64_t lora_decode_chain_soft_batch(int sf, int rdd, const float* llr, int64_t frames, int64_t sym_count,
                                     int64_t sym_stride, int64_t nbytes, uint8_t* payload, int64_t payload_stride,
                                     int32_t* corrected, int device, void* stream) {
  if (!chain_params_ok(sf, rdd, nbytes))
    return set_last_error(LORA_EINVAL, "sf must be in 6..12, rdd in 0..4, nbytes in 0..255");
  if (frames < 0 || sym_count < 0) return set_last_error(LORA_EINVAL, "bad frames / sym_count");
  if (sym_stride < sym_count) return set_last_error(LORA_EINVAL, "sym_stride smaller than sym_count");
  if (payload_stride < nbytes) return set_last_error(LORA_EINVAL, "payload_stride smaller than nbytes");
  if (2 * nbytes > sym_count / (4 + rdd) * sf)
    return set_last_error(LORA_ERANGE, "nbytes needs more codewords than sym_count yields");
  if (frames == 0) return nbytes;
  if (nbytes > 0 && (!llr || !payload)) return set_last_error(LORA_EINVAL, "null buffer");
  if (nbytes == 0 && !corrected) return nbytes;  // nothing to write
  ChainArgs a{};
  a.sf = sf;
  a.rdd = rdd;
  a.nbytes = (int)nbytes;
  a.lg = group_lg(nbytes);
  a.frames = frames;
  a.sym_stride = sym_stride;
  a.pay_stride = payload_stride;
  a.pay_out = payload;
  a.err = corrected;
  const SoftArgs sa{a, llr};
  switch (rdd) {
    case 0: return launch_frames(k_soft_chain_decode<0>, sa, frames, a.lg, device, stream, nbytes);
    case 1: return launch_frames(k_soft_chain_decode<1>, sa, frames, a.lg, device, stream, nbytes);
    case 2: return launch_frames(k_soft_chain_decode<2>, sa, frames, a.lg, device, stream, nbytes);
    case 3: return launch_frames(k_soft_chain_decode<3>, sa, frames, a.lg, device, stream, nbytes);
    default: return launch_frames(k_soft_chain_decode<4>, sa, frames, a.lg, device, stream, nbytes);
  }
}

int64_t lora_encode_chain_batch(int sf, int rdd, const uint8_t* payload, int64_t frames, int64_t nbytes,
                                int64_t payload_stride, uint16_t* symbols, int64_t sym_stride, int device,
                                void* stream) {
  if (!chain_params_ok(sf, rdd, nbytes))
    return set_last_error(LORA_EINVAL, "sf must be in 6..12, rdd in 0..4, nbytes in 0..255");
  if (frames < 0) return set_last_error(LORA_EINVAL, "bad frames");
  const int64_t nsym = chain_blocks(sf, nbytes) * (4 + rdd);
  if (payload_stride < nbytes) return set_last_error(LORA_EINVAL, "payload_stride smaller than nbytes");
  if (sym_stride < nsym) return set_last_error(LORA_EINVAL, "sym_stride smaller than the symbols per frame");
  if (frames == 0 || nsym == 0) return nsym;
  if (!symbols || !payload) return set_last_error(LORA_EINVAL, "null buffer");
  ChainArgs a{};
  a.sf = sf;
  a.rdd = rdd;
  a.nbytes = (int)nbytes;
  a.lg = group_lg(nsym);
  a.nsym = (int)nsym;
  a.ncw = (int)(chain_blocks(sf, nbytes) * sf);
  a.frames = frames;
  a.sym_stride = sym_stride;
  a.pay_stride = payload_stride;
  a.pay_in = payload;
  a.sym_out = symbols;
  if ((int64_t)(kBlock >> a.lg) * a.ncw > kChainEncLds) return set_last_error(LORA_EINVAL, "frame too long");
  return launch_frames(k_codec_chain_encode, a, frames, a.lg, device, stream, nsym);
}

namespace {
bool frame_params_ok(int sf, int rdd, int64_t nbytes, int crc) {
  return sf >= 7 && sf <= 12 && rdd >= 0 && rdd <= 4 && nbytes >= 0 && nbytes <= kMaxPayload && (crc == 0 || crc == 1);
}
const char* const kFrameParams = "sf must be in 7..12, rdd in 0..4, nbytes in 0..255, crc 0 or 1";
}  // namespace

int64_t lora_frame_symbols(int sf, int rdd, int64_t nbytes, int crc) {
  if (!frame_params_ok(sf, rdd, nbytes, crc)) return set_last_error(LORA_EINVAL, kFrameParams);
  return frame_nsym(sf, rdd, (int)nbytes, crc);
}

int64_t lora_encode_frame_batch(int sf, int rdd, int crc, const uint8_t* payload, int64_t frames, int64_t max_bytes,
                                int64_t payload_stride, const int32_t* nbytes, uint16_t* symbols,
                                int64_t sym_stride, int32_t* nsym, int device, void* stream) {
  if (!frame_params_ok(sf, rdd, max_bytes, crc)) return set_last_error(LORA_EINVAL, kFrameParams);
  if (frames < 0) return set_last_error(LORA_EINVAL, "bad frames");
  const int64_t cols = frame_nsym(sf, rdd, (int)max_bytes, crc);
  if (payload_stride < max_bytes) return set_last_error(LORA_EINVAL, "payload_stride smaller than max_bytes");
  if (sym_stride < cols) return set_last_error(LORA_EINVAL, "sym_stride smaller than the symbols per frame");
  if (frames == 0) return cols;
  if (!symbols || (max_bytes > 0 && !payload)) return set_last_error(LORA_EINVAL, "null buffer");
  FrameEncArgs a{};
  a.sf = sf;
  a.rdd = rdd;
  a.crc = crc;
  a.max_bytes = (int)max_bytes;
  a.lg = group_lg(cols);
  a.cols = (int)cols;
  a.frames = frames;
  a.pay_stride = payload_stride;
  a.sym_stride = sym_stride;
  a.pay = payload;
  a.nbytes = nbytes;
  a.sym = symbols;
  a.nsym = nsym;
  return launch_frames(k_frame_encode, a, frames, a.lg, device, stream, cols);
}

int64_t lora_decode_frame_batch(int sf, const uint16_t* symbols, int64_t frames, int64_t sym_count,
                                int64_t sym_stride, const int32_t* avail, int32_t* status, int32_t* nbytes,
                                int32_t* rdd, int32_t* has_crc, int32_t* nsym, int32_t* errors, uint8_t* payload,
                                int64_t max_bytes, int64_t payload_stride, int device, void* stream) {
  if (sf < 7 || sf > 12) return set_last_error(LORA_EINVAL, "sf must be in 7..12");
  if (frames < 0 || sym_count < 0 || sym_count >= (int64_t(1) << 31))
    return set_last_error(LORA_EINVAL, "bad frames / sym_count");
  if (sym_stride < sym_count) return set_last_error(LORA_EINVAL, "sym_stride smaller than sym_count");
  if (!payload) max_bytes = 0;  // header-only mode
  if (max_bytes < 0 || max_bytes > kMaxPayload) return set_last_error(LORA_EINVAL, "max_bytes must be in 0..255");
  if (payload && payload_stride < max_bytes)
    return set_last_error(LORA_EINVAL, "payload_stride smaller than max_bytes");
  if (frames == 0) return max_bytes;
  if (sym_count > 0 && !symbols) return set_last_error(LORA_EINVAL, "null buffer");
  if (!payload && !status && !nbytes && !rdd && !has_crc && !nsym && !errors) return max_bytes;  // nothing to write
  FrameDecArgs a{};
  a.sf = sf;
  a.max_bytes = (int)max_bytes;
  a.lg = payload ? group_lg(max_bytes + 2) : 0;
  a.cols = (int)sym_count;
  a.frames = frames;
  a.sym_stride = sym_stride;
  a.pay_stride = payload_stride;
  a.sym = symbols;
  a.avail = avail;
  a.status = status;
  a.nbytes = nbytes;
  a.rdd = rdd;
  a.has_crc = has_crc;
  a.nsym = nsym;
  a.errors = errors;
  a.pay = payload;
  return launch_frames(k_frame_decode, a, frames, a.lg, device, stream, max_bytes);
}

int64_t lora_decode_frame_soft_batch(int sf, const float* llr, int64_t frames, int64_t sym_count,
                                     int64_t sym_stride, const int32_t* avail, int32_t* status, int32_t* nbytes,
                                     int32_t* rdd, int32_t* has_crc, int32_t* nsym, int32_t* corrected,
                                     int32_t* hdr_flips, int max_flips, uint8_t* payload, int64_t max_bytes,
                                     int64_t payload_stride, int device, void* stream) {
  if (sf < 7 || sf > 12) return set_last_error(LORA_EINVAL, "sf must be in 7..12");
  if (frames < 0 || sym_count < 0 || sym_count >= (int64_t(1) << 31))
    return set_last_error(LORA_EINVAL, "bad frames / sym_count");
  if (sym_stride < sym_count) return set_last_error(LORA_EINVAL, "sym_stride smaller than sym_count");
  if (max_flips < 0 || max_flips > 40) return set_last_error(LORA_EINVAL, "max_flips must be in 0..40");
  if (!payload) max_bytes = 0;  // header-only mode
  if (max_bytes < 0 || max_bytes > kMaxPayload) return set_last_error(LORA_EINVAL, "max_bytes must be in 0..255");
  if (payload && payload_stride < max_bytes)
    return set_last_error(LORA_EINVAL, "payload_stride smaller than max_bytes");
  if (frames == 0) return max_bytes;
  if (sym_count > 0 && !llr) return set_last_error(LORA_EINVAL, "null buffer");
  if (!payload && !status && !nbytes && !rdd && !has_crc && !nsym && !corrected && !hdr_flips)
    return max_bytes;  // nothing to write
  FrameSoftArgs a{};
  a.max_bytes = (int)max_bytes;
  a.max_flips = max_flips;
  a.lg = payload ? group_lg(max_bytes + 2) : 0;
  a.cols = (int)sym_count;
  a.frames = frames;
  a.sym_stride = sym_stride;
  a.pay_stride = payload_stride;
  a.llr = llr;
  a.avail = avail;
  a.status = status;
  a.nbytes = nbytes;
  a.rdd = rdd;
  a.has_crc = has_crc;
  a.nsym = nsym;
  a.corrected = corrected;
  a.hdr_flips = hdr_flips;
  a.pay = payload;
  switch (sf) {
    case 7: return launch_frames(k_frame_decode_soft<7>, a, frames, a.lg, device, stream, max_bytes);
    case 8: return launch_frames(k_frame_decode_soft<8>, a, frames, a.lg, device, stream, max_bytes);
    case 9: return launch_frames(k_frame_decode_soft<9>, a, frames, a.lg, device, stream, max_bytes);
    case 10: return launch_frames(k_frame_decode_soft<10>, a, frames, a.lg, device, stream, max_bytes);
    case 11: return launch_frames(k_frame_decode_soft<11>, a, frames, a.lg, device, stream, max_bytes);
    default: return launch_frames(k_frame_decode_soft<12>, a, frames, a.lg, device, stream, max_bytes);
  }
}
