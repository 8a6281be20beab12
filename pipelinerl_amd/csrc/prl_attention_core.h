// Device code shared by the packed attention kernels: the square form (prl_attention.hip: queries and keys are the same N
// tokens) and the sequence-parallel slice form (prl_attention_sp.hip: nq local queries at a global offset against nk keys).
// Staging into LDS, MFMA fragments, the tile store, one online-softmax step, the delta row sum, and the argument checks both
// sets of entry points make.  Everything here is inlined into its caller: the two files share arithmetic, not object code, so
// a slice whose offset is a multiple of 64 walks the same tiles in the same order as the square kernel and gives the same bits.
#pragma once

#include "prl_common.h"
#include "prl_optim_math.h"
#include "prl_osm.h"

#ifndef PRL_ATTN_BQ  // (prl_attention.hip states the two sizes itself, ahead of this header)
#define PRL_ATTN_BQ 64
#define PRL_ATTN_BK 64
#endif

namespace prl {
namespace attn {

using prl::osm::fast_exp2;
using prl::osm::kLn2;
using prl::osm::kLog2e;
using prl::osm::kNegBig;

constexpr int kBlk = 64;        // rows of a block and of a swept tile (PRL_ATTN_BQ == PRL_ATTN_BK)
constexpr int kThreads = 256;   // 4 waves x 16 rows
constexpr int kLdT = kBlk + 8;  // row length of a [.][64] LDS image: 144 bytes, 16-byte multiple, rows fall on different banks
constexpr float kVisible = -1.0e38f;  // a score above this is a visible one (masked ones are kNegBig)
static_assert(PRL_ATTN_BQ == kBlk && PRL_ATTN_BK == kBlk, "one tile size");

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__host__ __device__ inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
__host__ __device__ inline int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }
__host__ __device__ inline int64_t max64(int64_t a, int64_t b) { return a > b ? a : b; }

__device__ __forceinline__ bf16x8 as_frag(u32x4 v) { return __builtin_bit_cast(bf16x8, v); }
__device__ __forceinline__ bf16x8 lds_frag(const uint16_t* img, int ld, int row, int col) {
  return as_frag(*reinterpret_cast<const u32x4*>(img + row * ld + col));
}
__device__ __forceinline__ f32x4 mfma(bf16x8 a, bf16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ float max16(float v) {  // over the 16 lanes that share a C row
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float sum16(float v) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) v = v + __shfl_xor(v, o, 64);
  return v;
}

// Rows [r0, r0 + 64) of one head of a [N, H, D] array (src points at the head, st = token stride) into the row image
// rows[64][D + 8] and / or the transposed image cols[D][64 + 8].  A row outside [lo, hi) reads as zero and is not touched.
template <int D, bool ROWS, bool COLS>
__device__ __forceinline__ void stage(const uint16_t* __restrict__ src, int64_t st, int64_t r0, int64_t lo, int64_t hi, uint16_t* rows, uint16_t* cols) {
  constexpr int CH = D / 8;
  for (int i = threadIdx.x; i < kBlk * CH; i += kThreads) {
    const int row = i / CH, ch = i % CH;
    const int64_t g = r0 + row;
    u32x4 val = {0u, 0u, 0u, 0u};
    if (g >= lo && g < hi) val = *reinterpret_cast<const u32x4*>(src + g * st + ch * 8);
    if constexpr (ROWS) *reinterpret_cast<u32x4*>(rows + row * (D + 8) + ch * 8) = val;
    if constexpr (COLS) {
#pragma unroll
      for (int e = 0; e < 8; ++e) cols[(ch * 8 + e) * kLdT + row] = uint16_t(val[e >> 1] >> ((e & 1) * 16));
    }
  }
}

// The 16 rows of this wave as A fragments straight from global memory: lane (g, c) takes row0 + c, columns 32 kk + 8 g ..
template <int D>
__device__ __forceinline__ void row_frags(const uint16_t* __restrict__ src, int64_t st, int64_t row, int64_t n, int g, bf16x8 (&a)[D / 32]) {
#pragma unroll
  for (int kk = 0; kk < D / 32; ++kk) {
    u32x4 val = {0u, 0u, 0u, 0u};
    if (row < n) val = *reinterpret_cast<const u32x4*>(src + row * st + kk * 32 + g * 8);
    a[kk] = as_frag(val);
  }
}

// acc (this wave's 16 rows x D, C layout) x mul -> bf16 rows [16 w ..] of the image, then whole rows to dst [N, H, D] (dst at the head)
template <int D>
__device__ __forceinline__ void store_tile(const f32x4 (&acc)[D / 16], const float (&mul)[4], uint16_t* img, uint16_t* __restrict__ dst, int64_t st,
                                           int64_t r0, int64_t n) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  __syncthreads();  // the image's last readers are done
#pragma unroll
  for (int t = 0; t < D / 16; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) img[(16 * w + 4 * g + r) * (D + 8) + 16 * t + c] = prl_f32_to_bf16_rne(acc[t][r] * mul[r]);
  __syncthreads();
  constexpr int CH = D / 8;
  for (int i = threadIdx.x; i < kBlk * CH; i += kThreads) {
    const int row = i / CH, ch = i % CH;
    const int64_t gr = r0 + row;
    if (gr < n) *reinterpret_cast<u32x4*>(dst + gr * st + ch * 8) = *reinterpret_cast<const u32x4*>(img + row * (D + 8) + ch * 8);
  }
}

// One online-softmax step of the forward: this wave's 16 x 64 scores `s` of the key tile at k0 (global key index) against the
// running maximum m, sum lsum and output o of its rows; the unnormalised P goes to the wave's LDS tile p_w in bf16.  `row` and
// `rs` are the global index and the sequence start of the lane's 4 rows; a `whole` tile takes no mask arithmetic.  (The square
// forward carries the same lines written out in its loop: called from there the compiler schedules that kernel differently, and its
// compiled code is to stay what it was.  The operations and their order are these, so the bits are.)
template <int D>
__device__ __forceinline__ void softmax_step(const f32x4 (&s)[4], float scale2, bool whole, int64_t k0, int c, int g, const int64_t (&row)[4],
                                             const int64_t (&rs)[4], float (&m)[4], float (&lsum)[4], f32x4 (&o)[D / 16], uint16_t* p_w) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float y[4];
#pragma unroll
    for (int nn = 0; nn < 4; ++nn) {
      y[nn] = s[nn][r] * scale2;
      if (!whole) {
        const int64_t j = k0 + 16 * nn + c;
        y[nn] = (j >= rs[r] && j <= row[r]) ? y[nn] : kNegBig;
      }
    }
    const float mx = max16(fmaxf(fmaxf(y[0], y[1]), fmaxf(y[2], y[3])));
    const float mn = fmaxf(m[r], mx);
    const float alpha = fast_exp2(m[r] - mn);
    m[r] = mn;
    lsum[r] = lsum[r] * alpha;
#pragma unroll
    for (int t = 0; t < D / 16; ++t) o[t][r] = o[t][r] * alpha;
#pragma unroll
    for (int nn = 0; nn < 4; ++nn) {
      const float p = y[nn] > kVisible ? fast_exp2(y[nn] - mn) : 0.0f;
      lsum[r] = lsum[r] + p;
      p_w[(4 * g + r) * kLdT + 16 * nn + c] = prl_f32_to_bf16_rne(p);
    }
  }
}

// delta[h, t] = sum_d dO O over the n rows of contiguous [n, hq, D] arrays.  D / 8 lanes per (token, head) row, 16 bytes each;
// a lane's 8 products pairwise, the lanes by butterfly: one fixed order.
template <int D>
__device__ __forceinline__ void delta_rows(const uint16_t* __restrict__ o, const uint16_t* __restrict__ d_o, float* __restrict__ delta, int64_t n, int hq) {
  constexpr int L = D / 8;
  const int64_t r = (int64_t(blockIdx.x) * kThreads + threadIdx.x) / L;  // row = t * hq + h (whole groups of L lanes share a row)
  const int part = threadIdx.x % L;
  float acc = 0.0f;
  if (r < n * hq) {
    const u32x4 a = *reinterpret_cast<const u32x4*>(o + r * D + part * 8);
    const u32x4 b = *reinterpret_cast<const u32x4*>(d_o + r * D + part * 8);
    float p[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      p[2 * e] = __uint_as_float(a[e] << 16) * __uint_as_float(b[e] << 16);
      p[2 * e + 1] = __uint_as_float(a[e] & 0xffff0000u) * __uint_as_float(b[e] & 0xffff0000u);
    }
    acc = ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]));
  }
#pragma unroll
  for (int off = 1; off < L; off <<= 1) acc = acc + __shfl_xor(acc, off, 64);
  if (r < n * hq && part == 0) delta[(r % hq) * n + r / hq] = acc;
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
constexpr int64_t kMaxTokens = (int64_t(1) << 31) - 2 * kBlk;  // token indices and block starts fit int32

inline int check_shape(int64_t n, int64_t hq, int64_t hkv, int64_t d) {
  PRL_CHECK_ARG(n >= 0, "negative n %lld", (long long)n);
  PRL_CHECK_ARG(n <= kMaxTokens, "n %lld tokens do not fit the int32 segment table", (long long)n);
  PRL_CHECK_ARG(d == 64 || d == 128, "head size %lld: the kernels are built for 64 and 128", (long long)d);
  PRL_CHECK_ARG(hq > 0 && hkv > 0 && hq <= 65535, "heads (hq %lld, hkv %lld) must be positive and at most 65535", (long long)hq, (long long)hkv);
  PRL_CHECK_ARG(hq % hkv == 0, "hq %lld is not a multiple of hkv %lld", (long long)hq, (long long)hkv);
  return PRL_OK;
}

inline int check_operand(const char* name, const void* p, int64_t st, int64_t sh, int64_t d) {
  PRL_CHECK_ARG(p != nullptr, "%s is null", name);
  PRL_CHECK_ARG(prl::aligned16(p), "%s is not 16-byte aligned", name);
  PRL_CHECK_ARG(st >= d && sh >= 0, "%s: token stride %lld must be at least d and head stride %lld not negative", name, (long long)st, (long long)sh);
  PRL_CHECK_ARG(st % 8 == 0 && sh % 8 == 0, "%s: strides (%lld, %lld) break the 16-byte alignment of its rows", name, (long long)st, (long long)sh);
  return PRL_OK;
}

inline size_t workspace_need(int64_t n, int64_t hq) { return size_t((n * hq * 4 + 15) & ~int64_t(15)); }

}  // namespace attn
}  // namespace prl
