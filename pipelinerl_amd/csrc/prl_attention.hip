// Packed variable-length causal attention for the learner body: segment table, forward, backward.
//
// Tokens of a packed batch lie flat, N = B T of them; q is [N, Hq, D], k and v are [N, Hkv, D] (bf16, D contiguous, token and head
// strides in elements).  The segment table gives every token the first token of its sequence and one past the last:
//     key j is visible to query i   iff   seq_start[i] <= j <= i.
// seq_start is non-decreasing, so the keys a query block [q0, q1) can see lie in [seq_start[q0], q1): the key sweep starts at the
// key block that holds seq_start[q0] - blocks before it are never loaded (a skip, not a multiply by zero).
//
// All three matrix kernels share one shape: 256 threads = 4 waves, a workgroup owns a block of 64 rows (queries; keys in dK/dV),
// a wave 16 of them, and sweeps 64-row tiles of the other side through LDS.  Products are mfma_f32_16x16x32_bf16 through the
// compiler builtin.  Lane l = 16 g + c of a wave holds
//     A[row c][k = 8 g + 0..7],  B[k = 8 g + 0..7][col c],  C[row 4 g + r][col c]  (r = 0..3)
// so an operand whose summed index is contiguous in memory (q, k, v, dO by rows of D) is one 16-byte read per fragment, and an
// operand summed over its ROW index (V in P V, K in dS K, dO in P^T dO, Q in dS^T Q) is read from a transposed LDS image
// [D][64 + 8] written at staging.  P / dS go from the accumulator layout to the A layout through a wave-private LDS tile, rounded
// to bf16 once.  The row owner keeps its own fragments in registers for the whole sweep.
//
// Forward: online softmax in base 2 (prl_osm.h: y = s scale log2 e), running maximum and sum per row in fp32, O in fp32
// accumulators; lse = ln2 (M + log2 S).  A tile wholly inside one sequence and below the diagonal takes no mask arithmetic.
// Backward: three launches, no atomics.  (1) delta[h, t] = sum_d dO O.  (2) dK, dV: a workgroup per key block x KV head sweeps the
// queries [k0, seq_end[k1 - 1]) of its G query heads in index order; S^T and dP^T are computed with the key on the accumulator
// row, dK^T / dV^T never leave the accumulators.  (3) dQ: a workgroup per query block x query head sweeps the forward's keys and
// recomputes S and dP.  Seven products instead of five: the price of sums with one fixed order and no hand-off between workgroups.
// A finished 64 x D tile goes through LDS and leaves as whole 16-byte pieces of rows.
#define PRL_ATTN_BQ 64
#define PRL_ATTN_BK 64
#include "prl_attention_core.h"  // staging, fragments, the tile store, the delta row sum: shared with prl_attention_sp.hip

namespace {

using namespace prl::attn;

constexpr int kSegThreads = 1024;

// ---- segment table -----------------------------------------------------------------------------------------------------------
// One workgroup per batch row; a thread owns a run of consecutive tokens.  Pass 1 finds the last and the first sequence start of
// each run, an inclusive max / min scan over the runs carries them across, pass 2 writes.
__device__ __forceinline__ bool mask_zero(const void* mask, int mb, int64_t i) {
  if (mb == 1) return static_cast<const uint8_t*>(mask)[i] == 0;
  if (mb == 4) return static_cast<const int32_t*>(mask)[i] == 0;
  return static_cast<const int64_t*>(mask)[i] == 0;
}
__device__ __forceinline__ bool is_start(const int64_t* pos, const void* mask, int mb, int64_t base, int c) {
  if (c == 0) return true;
  const int64_t i = base + c;
  if (pos != nullptr && pos[i] != pos[i - 1] + 1) return true;
  if (mask != nullptr && (mask_zero(mask, mb, i) || mask_zero(mask, mb, i - 1))) return true;
  return false;
}

__global__ __launch_bounds__(kSegThreads) void attn_segments_kernel(const int64_t* __restrict__ pos, const void* __restrict__ mask, int mb, int T,
                                                                   int32_t* __restrict__ seq_start, int32_t* __restrict__ seq_end) {
  __shared__ int last[kSegThreads], first[kSegThreads];
  const int tid = threadIdx.x;
  const int64_t base = int64_t(blockIdx.x) * T;
  const int run = int(ceil_div(T, kSegThreads));
  const int c0 = int(min64(int64_t(tid) * run, T)), c1 = int(min64(int64_t(c0) + run, T));
  int l = -1, f = T;
  for (int c = c0; c < c1; ++c)
    if (is_start(pos, mask, mb, base, c)) {
      l = c;
      if (f == T) f = c;
    }
  last[tid] = l, first[tid] = f;
  __syncthreads();
  for (int off = 1; off < kSegThreads; off <<= 1) {
    const int a = tid >= off ? last[tid - off] : -1;
    const int b = tid + off < kSegThreads ? first[tid + off] : T;
    __syncthreads();
    last[tid] = max(last[tid], a), first[tid] = min(first[tid], b);
    __syncthreads();
  }
  int cur = tid > 0 ? last[tid - 1] : 0;
  for (int c = c0; c < c1; ++c) {
    if (is_start(pos, mask, mb, base, c)) cur = c;
    seq_start[base + c] = int32_t(base + cur);
  }
  cur = tid + 1 < kSegThreads ? first[tid + 1] : T;
  for (int c = c1 - 1; c >= c0; --c) {
    seq_end[base + c] = int32_t(base + cur);
    if (is_start(pos, mask, mb, base, c)) cur = c;
  }
}

// ---- forward -------------------------------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(kThreads) void attn_fwd_kernel(const uint16_t* __restrict__ q, int64_t qst, int64_t qsh, const uint16_t* __restrict__ k, int64_t kst,
                                                            int64_t ksh, const uint16_t* __restrict__ v, int64_t vst, int64_t vsh, float scale2,
                                                            const int32_t* __restrict__ seq_start, uint16_t* __restrict__ out, float* __restrict__ lse,
                                                            int64_t n, int hq, int group) {
  constexpr int LDD = D + 8;
  __shared__ __attribute__((aligned(16))) uint16_t k_rows[kBlk * LDD];
  __shared__ __attribute__((aligned(16))) uint16_t v_cols[D * kLdT];
  __shared__ __attribute__((aligned(16))) uint16_t p_img[4 * 16 * kLdT];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int h = blockIdx.y, kvh = h / group;
  const int64_t q0 = int64_t(blockIdx.x) * kBlk, q1 = min64(q0 + kBlk, n);
  const uint16_t* kh = k + int64_t(kvh) * ksh;
  const uint16_t* vh = v + int64_t(kvh) * vsh;
  bf16x8 qa[D / 32];
  row_frags<D>(q + int64_t(h) * qsh, qst, q0 + 16 * w + c, n, g, qa);
  int64_t row[4];
  int64_t rs[4];
  float m[4], lsum[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    row[r] = q0 + 16 * w + 4 * g + r;
    rs[r] = row[r] < n ? int64_t(seq_start[row[r]]) : (int64_t(1) << 62);
    m[r] = kNegBig, lsum[r] = 0.0f;
  }
  f32x4 o[D / 16];
#pragma unroll
  for (int t = 0; t < D / 16; ++t) o[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  const int64_t lo = seq_start[q0], ss_last = seq_start[q1 - 1];
  uint16_t* p_w = p_img + w * 16 * kLdT;

  for (int64_t k0 = lo / kBlk * kBlk; k0 < q1; k0 += kBlk) {
    __syncthreads();
    stage<D, true, false>(kh, kst, k0, lo, q1, k_rows, nullptr);
    stage<D, false, true>(vh, vst, k0, lo, q1, nullptr, v_cols);
    __syncthreads();
    f32x4 s[4];
#pragma unroll
    for (int nn = 0; nn < 4; ++nn) {
      s[nn] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int kk = 0; kk < D / 32; ++kk) s[nn] = mfma(qa[kk], lds_frag(k_rows, LDD, 16 * nn + c, 32 * kk + 8 * g), s[nn]);
    }
    const bool whole = k0 >= ss_last && k0 + kBlk - 1 <= q0;  // inside one sequence, below the diagonal
    // (softmax_step of prl_attention_core.h, written out: this kernel compiles to the schedule it had before the step was shared)
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
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < kBlk / 32; ++kk) {
      const bf16x8 pa = lds_frag(p_w, kLdT, c, 32 * kk + 8 * g);
#pragma unroll
      for (int t = 0; t < D / 16; ++t) o[t] = mfma(pa, lds_frag(v_cols, kLdT, 16 * t + c, 32 * kk + 8 * g), o[t]);
    }
  }
  float inv[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float l = sum16(lsum[r]);
    inv[r] = l > 0.0f ? 1.0f / l : 0.0f;
    if (c == 0 && row[r] < n) lse[int64_t(h) * n + row[r]] = kLn2 * (m[r] + log2f(l));
  }
  store_tile<D>(o, inv, k_rows, out + int64_t(h) * D, int64_t(hq) * D, q0, n);
}

// ---- backward 1: delta = rowsum(dO * O) ----------------------------------------------------------------------------------------
// (delta_rows of prl_attention_core.h: one fixed order.)
template <int D>
__global__ __launch_bounds__(kThreads) void attn_delta_kernel(const uint16_t* __restrict__ o, const uint16_t* __restrict__ d_o, float* __restrict__ delta,
                                                              int64_t n, int hq) {
  delta_rows<D>(o, d_o, delta, n, hq);
}

// ---- backward 2: dK, dV ----------------------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(kThreads) void attn_dkv_kernel(const uint16_t* __restrict__ q, int64_t qst, int64_t qsh, const uint16_t* __restrict__ k, int64_t kst,
                                                            int64_t ksh, const uint16_t* __restrict__ v, int64_t vst, int64_t vsh, float scale, float scale2,
                                                            const int32_t* __restrict__ seq_start, const int32_t* __restrict__ seq_end,
                                                            const float* __restrict__ lse, const float* __restrict__ delta, const uint16_t* __restrict__ d_o,
                                                            uint16_t* __restrict__ dk, uint16_t* __restrict__ dv, int64_t n, int hq, int hkv, int group) {
  constexpr int LDD = D + 8;
  __shared__ __attribute__((aligned(16))) uint16_t q_rows[kBlk * LDD];
  __shared__ __attribute__((aligned(16))) uint16_t do_rows[kBlk * LDD];
  __shared__ __attribute__((aligned(16))) uint16_t q_cols[D * kLdT];
  __shared__ __attribute__((aligned(16))) uint16_t do_cols[D * kLdT];
  __shared__ __attribute__((aligned(16))) uint16_t p_img[4 * 16 * kLdT];
  __shared__ __attribute__((aligned(16))) uint16_t ds_img[4 * 16 * kLdT];
  __shared__ float lse2_s[kBlk], delta_s[kBlk];
  __shared__ int64_t start_s[kBlk];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int kvh = blockIdx.y;
  const int64_t k0 = int64_t(blockIdx.x) * kBlk, k1 = min64(k0 + kBlk, n);
  bf16x8 ka[D / 32], va[D / 32];
  row_frags<D>(k + int64_t(kvh) * ksh, kst, k0 + 16 * w + c, n, g, ka);
  row_frags<D>(v + int64_t(kvh) * vsh, vst, k0 + 16 * w + c, n, g, va);
  int64_t key[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) key[r] = k0 + 16 * w + 4 * g + r;
  f32x4 acc_k[D / 16], acc_v[D / 16];
#pragma unroll
  for (int t = 0; t < D / 16; ++t) acc_k[t] = acc_v[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  const int64_t q_end = seq_end[k1 - 1];  // no query from here on sees a key of this block
  uint16_t* p_w = p_img + w * 16 * kLdT;
  uint16_t* ds_w = ds_img + w * 16 * kLdT;

  for (int hh = 0; hh < group; ++hh) {
    const int h = kvh * group + hh;
    const uint16_t* qh = q + int64_t(h) * qsh;
    const uint16_t* doh = d_o + int64_t(h) * D;
    for (int64_t q0 = k0; q0 < q_end; q0 += kBlk) {
      __syncthreads();
      stage<D, true, true>(qh, qst, q0, k0, q_end, q_rows, q_cols);
      stage<D, true, true>(doh, int64_t(hq) * D, q0, k0, q_end, do_rows, do_cols);
      if (threadIdx.x < kBlk) {
        const int64_t i = q0 + threadIdx.x;
        const bool in = i < q_end;
        lse2_s[threadIdx.x] = in ? lse[int64_t(h) * n + i] * kLog2e : 0.0f;
        delta_s[threadIdx.x] = in ? delta[int64_t(h) * n + i] : 0.0f;
        start_s[threadIdx.x] = in ? int64_t(seq_start[i]) : (int64_t(1) << 62);
      }
      __syncthreads();
      // a tile whose queries all see all of the block's keys: the last query starts at or before k0, the first is past k1 - 1
      const bool whole = q0 + kBlk <= q_end && start_s[kBlk - 1] <= k0 && q0 >= k0 + kBlk - 1 && k1 == k0 + kBlk;
#pragma unroll
      for (int nn = 0; nn < 4; ++nn) {
        f32x4 s = f32x4{0.0f, 0.0f, 0.0f, 0.0f}, dp = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int kk = 0; kk < D / 32; ++kk) {
          s = mfma(ka[kk], lds_frag(q_rows, LDD, 16 * nn + c, 32 * kk + 8 * g), s);
          dp = mfma(va[kk], lds_frag(do_rows, LDD, 16 * nn + c, 32 * kk + 8 * g), dp);
        }
        const int qi = 16 * nn + c;
        const int64_t i = q0 + qi, st = start_s[qi];
        const float l2 = lse2_s[qi], dl = delta_s[qi];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool vis = whole || (key[r] >= st && key[r] <= i);
          const float p = vis ? fast_exp2(s[r] * scale2 - l2) : 0.0f;
          const float ds = vis ? p * (dp[r] - dl) : 0.0f;
          p_w[(4 * g + r) * kLdT + qi] = prl_f32_to_bf16_rne(p);
          ds_w[(4 * g + r) * kLdT + qi] = prl_f32_to_bf16_rne(ds);
        }
      }
      __syncthreads();
#pragma unroll
      for (int kk = 0; kk < kBlk / 32; ++kk) {
        const bf16x8 pa = lds_frag(p_w, kLdT, c, 32 * kk + 8 * g);
        const bf16x8 da = lds_frag(ds_w, kLdT, c, 32 * kk + 8 * g);
#pragma unroll
        for (int t = 0; t < D / 16; ++t) {
          acc_v[t] = mfma(pa, lds_frag(do_cols, kLdT, 16 * t + c, 32 * kk + 8 * g), acc_v[t]);
          acc_k[t] = mfma(da, lds_frag(q_cols, kLdT, 16 * t + c, 32 * kk + 8 * g), acc_k[t]);
        }
      }
    }
  }
  const float one[4] = {1.0f, 1.0f, 1.0f, 1.0f}, sc[4] = {scale, scale, scale, scale};
  store_tile<D>(acc_v, one, do_rows, dv + int64_t(kvh) * D, int64_t(hkv) * D, k0, n);
  store_tile<D>(acc_k, sc, q_rows, dk + int64_t(kvh) * D, int64_t(hkv) * D, k0, n);
}

// ---- backward 3: dQ ------------------------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(kThreads) void attn_dq_kernel(const uint16_t* __restrict__ q, int64_t qst, int64_t qsh, const uint16_t* __restrict__ k, int64_t kst,
                                                           int64_t ksh, const uint16_t* __restrict__ v, int64_t vst, int64_t vsh, float scale, float scale2,
                                                           const int32_t* __restrict__ seq_start, const float* __restrict__ lse, const float* __restrict__ delta,
                                                           const uint16_t* __restrict__ d_o, uint16_t* __restrict__ dq, int64_t n, int hq, int group) {
  constexpr int LDD = D + 8;
  __shared__ __attribute__((aligned(16))) uint16_t k_rows[kBlk * LDD];
  __shared__ __attribute__((aligned(16))) uint16_t v_rows[kBlk * LDD];
  __shared__ __attribute__((aligned(16))) uint16_t k_cols[D * kLdT];
  __shared__ __attribute__((aligned(16))) uint16_t ds_img[4 * 16 * kLdT];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int h = blockIdx.y, kvh = h / group;
  const int64_t q0 = int64_t(blockIdx.x) * kBlk, q1 = min64(q0 + kBlk, n);
  const uint16_t* kh = k + int64_t(kvh) * ksh;
  const uint16_t* vh = v + int64_t(kvh) * vsh;
  bf16x8 qa[D / 32], da[D / 32];
  row_frags<D>(q + int64_t(h) * qsh, qst, q0 + 16 * w + c, n, g, qa);
  row_frags<D>(d_o + int64_t(h) * D, int64_t(hq) * D, q0 + 16 * w + c, n, g, da);
  int64_t row[4], rs[4];
  float l2[4], dl[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    row[r] = q0 + 16 * w + 4 * g + r;
    const bool in = row[r] < n;
    rs[r] = in ? int64_t(seq_start[row[r]]) : (int64_t(1) << 62);
    l2[r] = in ? lse[int64_t(h) * n + row[r]] * kLog2e : 0.0f;
    dl[r] = in ? delta[int64_t(h) * n + row[r]] : 0.0f;
  }
  f32x4 acc[D / 16];
#pragma unroll
  for (int t = 0; t < D / 16; ++t) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  const int64_t lo = seq_start[q0], ss_last = seq_start[q1 - 1];
  uint16_t* ds_w = ds_img + w * 16 * kLdT;

  for (int64_t k0 = lo / kBlk * kBlk; k0 < q1; k0 += kBlk) {
    __syncthreads();
    stage<D, true, true>(kh, kst, k0, lo, q1, k_rows, k_cols);
    stage<D, true, false>(vh, vst, k0, lo, q1, v_rows, nullptr);
    __syncthreads();
    const bool whole = k0 >= ss_last && k0 + kBlk - 1 <= q0 && q1 == q0 + kBlk;
#pragma unroll
    for (int nn = 0; nn < 4; ++nn) {
      f32x4 s = f32x4{0.0f, 0.0f, 0.0f, 0.0f}, dp = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int kk = 0; kk < D / 32; ++kk) {
        s = mfma(qa[kk], lds_frag(k_rows, LDD, 16 * nn + c, 32 * kk + 8 * g), s);
        dp = mfma(da[kk], lds_frag(v_rows, LDD, 16 * nn + c, 32 * kk + 8 * g), dp);
      }
      const int64_t j = k0 + 16 * nn + c;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool vis = whole || (j >= rs[r] && j <= row[r]);
        const float p = vis ? fast_exp2(s[r] * scale2 - l2[r]) : 0.0f;
        const float ds = vis ? p * (dp[r] - dl[r]) : 0.0f;
        ds_w[(4 * g + r) * kLdT + 16 * nn + c] = prl_f32_to_bf16_rne(ds);
      }
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < kBlk / 32; ++kk) {
      const bf16x8 sa = lds_frag(ds_w, kLdT, c, 32 * kk + 8 * g);
#pragma unroll
      for (int t = 0; t < D / 16; ++t) acc[t] = mfma(sa, lds_frag(k_cols, kLdT, 16 * t + c, 32 * kk + 8 * g), acc[t]);
    }
  }
  const float sc[4] = {scale, scale, scale, scale};
  store_tile<D>(acc, sc, k_rows, dq + int64_t(h) * D, int64_t(hq) * D, q0, n);
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
}  // namespace

extern "C" int prl_attn_segments(int64_t batch, int64_t t, const int64_t* position_ids, const void* attention_mask, int32_t mask_elem_bytes,
                                 int32_t* seq_start, int32_t* seq_end, prl_stream_t stream) {
  PRL_CHECK_ARG(batch >= 0 && t >= 0, "negative size (batch %lld, t %lld)", (long long)batch, (long long)t);
  int64_t n = 0;
  PRL_CHECK_ARG(!__builtin_mul_overflow(batch, t, &n) && n <= kMaxTokens, "batch %lld x t %lld tokens do not fit the int32 segment table", (long long)batch,
                (long long)t);
  PRL_CHECK_ARG(attention_mask == nullptr || mask_elem_bytes == 1 || mask_elem_bytes == 4 || mask_elem_bytes == 8,
                "mask_elem_bytes %d: the mask is bool / uint8 (1), int32 (4) or int64 (8)", mask_elem_bytes);
  if (n == 0) return PRL_OK;
  PRL_CHECK_ARG(seq_start != nullptr && seq_end != nullptr, "null pointer (seq_start %p, seq_end %p)", (void*)seq_start, (void*)seq_end);
  hipLaunchKernelGGL(attn_segments_kernel, dim3(unsigned(batch)), dim3(kSegThreads), 0, static_cast<hipStream_t>(stream), position_ids, attention_mask,
                     int(mask_elem_bytes), int(t), seq_start, seq_end);
  PRL_LAUNCH_CHECK("attn_segments_kernel");
  return PRL_OK;
}

extern "C" int prl_attn_workspace_bytes(int64_t n, int64_t hq, size_t* bytes) {
  PRL_CHECK_ARG(bytes != nullptr, "bytes is null");
  PRL_CHECK_ARG(n >= 0 && n <= kMaxTokens, "n %lld is negative or does not fit the int32 segment table", (long long)n);
  PRL_CHECK_ARG(hq > 0 && hq <= 65535, "hq %lld must be positive and at most 65535", (long long)hq);
  *bytes = workspace_need(n, hq);
  return PRL_OK;
}

extern "C" int prl_attn_varlen_fwd(int64_t n, int64_t hq, int64_t hkv, int64_t d, const void* q, int64_t q_stride_t, int64_t q_stride_h, const void* k,
                                   int64_t k_stride_t, int64_t k_stride_h, const void* v, int64_t v_stride_t, int64_t v_stride_h, float scale,
                                   const int32_t* seq_start, const int32_t* seq_end, void* out, float* lse, prl_stream_t stream) {
  if (int rc = check_shape(n, hq, hkv, d)) return rc;
  if (n == 0) return PRL_OK;
  if (int rc = check_operand("q", q, q_stride_t, q_stride_h, d)) return rc;
  if (int rc = check_operand("k", k, k_stride_t, k_stride_h, d)) return rc;
  if (int rc = check_operand("v", v, v_stride_t, v_stride_h, d)) return rc;
  PRL_CHECK_ARG(seq_start != nullptr && seq_end != nullptr && lse != nullptr, "null pointer (seq_start %p, seq_end %p, lse %p)", (const void*)seq_start,
                (const void*)seq_end, (void*)lse);
  PRL_CHECK_ARG(out != nullptr && prl::aligned16(out), "out %p is null or not 16-byte aligned", out);
  const dim3 grid(unsigned(ceil_div(n, kBlk)), unsigned(hq)), block(kThreads);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const float scale2 = scale * kLog2e;
#define PRL_ATTN_FWD(DD)                                                                                                                                  \
  hipLaunchKernelGGL(attn_fwd_kernel<DD>, grid, block, 0, st, static_cast<const uint16_t*>(q), q_stride_t, q_stride_h, static_cast<const uint16_t*>(k),   \
                     k_stride_t, k_stride_h, static_cast<const uint16_t*>(v), v_stride_t, v_stride_h, scale2, seq_start, static_cast<uint16_t*>(out), lse, \
                     n, int(hq), int(hq / hkv))
  if (d == 64) PRL_ATTN_FWD(64);
  else PRL_ATTN_FWD(128);
#undef PRL_ATTN_FWD
  PRL_LAUNCH_CHECK("attn_fwd_kernel");
  return PRL_OK;
}

extern "C" int prl_attn_varlen_bwd(int64_t n, int64_t hq, int64_t hkv, int64_t d, const void* q, int64_t q_stride_t, int64_t q_stride_h, const void* k,
                                   int64_t k_stride_t, int64_t k_stride_h, const void* v, int64_t v_stride_t, int64_t v_stride_h, float scale,
                                   const int32_t* seq_start, const int32_t* seq_end, const void* out, const float* lse, const void* grad_out, void* grad_q,
                                   void* grad_k, void* grad_v, void* workspace, size_t workspace_bytes, prl_stream_t stream) {
  if (int rc = check_shape(n, hq, hkv, d)) return rc;
  if (n == 0) return PRL_OK;
  if (int rc = check_operand("q", q, q_stride_t, q_stride_h, d)) return rc;
  if (int rc = check_operand("k", k, k_stride_t, k_stride_h, d)) return rc;
  if (int rc = check_operand("v", v, v_stride_t, v_stride_h, d)) return rc;
  PRL_CHECK_ARG(seq_start != nullptr && seq_end != nullptr && lse != nullptr, "null pointer (seq_start %p, seq_end %p, lse %p)", (const void*)seq_start,
                (const void*)seq_end, (const void*)lse);
  PRL_CHECK_ARG(out != nullptr && grad_out != nullptr && grad_q != nullptr && grad_k != nullptr && grad_v != nullptr,
                "null pointer (out %p, grad_out %p, grad_q %p, grad_k %p, grad_v %p)", out, grad_out, grad_q, grad_k, grad_v);
  PRL_CHECK_ARG(prl::aligned16(out) && prl::aligned16(grad_out) && prl::aligned16(grad_q) && prl::aligned16(grad_k) && prl::aligned16(grad_v),
                "out and the gradients must be 16-byte aligned");
  const size_t need = workspace_need(n, hq);
  PRL_CHECK_ARG(workspace != nullptr && prl::aligned16(workspace), "workspace %p is null or not 16-byte aligned", workspace);
  PRL_CHECK_ARG(workspace_bytes >= need, "workspace too small: %zu < %zu bytes", workspace_bytes, need);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const float scale2 = scale * kLog2e;
  float* delta = static_cast<float*>(workspace);
  const int group = int(hq / hkv);
  const dim3 block(kThreads);
  PRL_CHECK_ARG(ceil_div(n * hq * (d / 8), kThreads) < (int64_t(1) << 31), "n %lld x hq %lld rows are too many for one launch", (long long)n, (long long)hq);
  const dim3 grid_delta(unsigned(ceil_div(n * hq * (d / 8), kThreads)));
  const dim3 grid_kv(unsigned(ceil_div(n, kBlk)), unsigned(hkv)), grid_q(unsigned(ceil_div(n, kBlk)), unsigned(hq));
  const uint16_t *qp = static_cast<const uint16_t*>(q), *kp = static_cast<const uint16_t*>(k), *vp = static_cast<const uint16_t*>(v);
  const uint16_t *op = static_cast<const uint16_t*>(out), *gp = static_cast<const uint16_t*>(grad_out);
#define PRL_ATTN_BWD(DD)                                                                                                                                    \
  do {                                                                                                                                                      \
    hipLaunchKernelGGL(attn_delta_kernel<DD>, grid_delta, block, 0, st, op, gp, delta, n, int(hq));                                                         \
    PRL_LAUNCH_CHECK("attn_delta_kernel");                                                                                                                  \
    hipLaunchKernelGGL(attn_dkv_kernel<DD>, grid_kv, block, 0, st, qp, q_stride_t, q_stride_h, kp, k_stride_t, k_stride_h, vp, v_stride_t, v_stride_h,      \
                       scale, scale2, seq_start, seq_end, lse, delta, gp, static_cast<uint16_t*>(grad_k), static_cast<uint16_t*>(grad_v), n, int(hq),      \
                       int(hkv), group);                                                                                                                    \
    PRL_LAUNCH_CHECK("attn_dkv_kernel");                                                                                                                    \
    hipLaunchKernelGGL(attn_dq_kernel<DD>, grid_q, block, 0, st, qp, q_stride_t, q_stride_h, kp, k_stride_t, k_stride_h, vp, v_stride_t, v_stride_h, scale, \
                       scale2, seq_start, lse, delta, gp, static_cast<uint16_t*>(grad_q), n, int(hq), group);                                               \
    PRL_LAUNCH_CHECK("attn_dq_kernel");                                                                                                                     \
  } while (0)
  if (d == 64) PRL_ATTN_BWD(64);
  else PRL_ATTN_BWD(128);
#undef PRL_ATTN_BWD
  return PRL_OK;
}
