// Sequence-parallel packed attention: the slice form of the kernels of prl_attention.hip.
//
// A packed row of nk tokens is cut into P contiguous slices, one per rank.  A rank keeps the nq queries of its slice - local
// query i is global token q_off + i - and attends them to the keys of the whole gathered row: k, v, seq_start, seq_end cover all
// nk tokens, and
//     key j is visible to local query i   iff   seq_start[q_off + i] <= j <= q_off + i.
// Forward and dQ are the square kernels with the query rows addressed locally and everything else globally: a workgroup per 64
// LOCAL query rows per query head sweeps the key tiles from the one that holds seq_start[q_off + q0] to the diagonal.  Key tiles
// stay on the global 64-grid, so a slice whose q_off is a multiple of 64 walks the square kernel's tiles in the square kernel's
// order and gives its bits; any other offset only makes a query block straddle two diagonal tiles.
// dK / dV: a workgroup per key block of the WHOLE row per KV head sweeps the local queries [max(k0, q_off), min(seq_end[k1 - 1],
// q_off + nq)) of its G query heads in index order and writes fp32 partials [nk, hkv, d].  A key block no local query can see has
// an empty sweep and writes its zero accumulators: the whole buffer is defined on return without a memset launch.  The partials
// of the P ranks are summed in rank order in fp32 and rounded to bf16 once (attn_slice_fold_kernel): a bf16 partial would add a
// rounding per rank.  No atomics anywhere; two runs give the same bits.
#include "prl_attention_core.h"

namespace {

using namespace prl::attn;

// ---- forward -------------------------------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(kThreads) void attn_slice_fwd_kernel(const uint16_t* __restrict__ q, int64_t qst, int64_t qsh, const uint16_t* __restrict__ k,
                                                                  int64_t kst, int64_t ksh, const uint16_t* __restrict__ v, int64_t vst, int64_t vsh,
                                                                  float scale2, const int32_t* __restrict__ seq_start, uint16_t* __restrict__ out,
                                                                  float* __restrict__ lse, int64_t nq, int64_t q_off, int hq, int group) {
  constexpr int LDD = D + 8;
  __shared__ __attribute__((aligned(16))) uint16_t k_rows[kBlk * LDD];
  __shared__ __attribute__((aligned(16))) uint16_t v_cols[D * kLdT];
  __shared__ __attribute__((aligned(16))) uint16_t p_img[4 * 16 * kLdT];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int h = blockIdx.y, kvh = h / group;
  const int64_t l0 = int64_t(blockIdx.x) * kBlk, l1 = min64(l0 + kBlk, nq);  // local rows
  const int64_t q0 = q_off + l0, q1 = q_off + l1;                            // the same rows, global
  const uint16_t* kh = k + int64_t(kvh) * ksh;
  const uint16_t* vh = v + int64_t(kvh) * vsh;
  bf16x8 qa[D / 32];
  row_frags<D>(q + int64_t(h) * qsh, qst, l0 + 16 * w + c, nq, g, qa);
  int64_t lrow[4], row[4], rs[4];
  float m[4], lsum[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    lrow[r] = l0 + 16 * w + 4 * g + r;
    row[r] = q_off + lrow[r];
    rs[r] = lrow[r] < nq ? int64_t(seq_start[row[r]]) : (int64_t(1) << 62);
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
    softmax_step<D>(s, scale2, whole, k0, c, g, row, rs, m, lsum, o, p_w);
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
    if (c == 0 && lrow[r] < nq) lse[int64_t(h) * nq + lrow[r]] = kLn2 * (m[r] + log2f(l));
  }
  store_tile<D>(o, inv, k_rows, out + int64_t(h) * D, int64_t(hq) * D, l0, nq);
}

// ---- backward 1: delta over the local rows ---------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(kThreads) void attn_slice_delta_kernel(const uint16_t* __restrict__ o, const uint16_t* __restrict__ d_o,
                                                                    float* __restrict__ delta, int64_t nq, int hq) {
  delta_rows<D>(o, d_o, delta, nq, hq);
}

// ---- backward 2: the fp32 partials of dK, dV over the whole row --------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(kThreads) void attn_slice_dkv_kernel(const uint16_t* __restrict__ q, int64_t qst, int64_t qsh, const uint16_t* __restrict__ k,
                                                                  int64_t kst, int64_t ksh, const uint16_t* __restrict__ v, int64_t vst, int64_t vsh,
                                                                  float scale, float scale2, const int32_t* __restrict__ seq_start,
                                                                  const int32_t* __restrict__ seq_end, const float* __restrict__ lse,
                                                                  const float* __restrict__ delta, const uint16_t* __restrict__ d_o,
                                                                  float* __restrict__ dk_part, float* __restrict__ dv_part, int64_t nq, int64_t nk,
                                                                  int64_t q_off, int hq, int hkv, int group) {
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
  const int64_t k0 = int64_t(blockIdx.x) * kBlk, k1 = min64(k0 + kBlk, nk);
  const int64_t q_hi = q_off + nq;  // one past the last local query, global: no key from here on is visible to this slice
  bf16x8 ka[D / 32], va[D / 32];
  row_frags<D>(k + int64_t(kvh) * ksh, kst, k0 + 16 * w + c, q_hi, g, ka);
  row_frags<D>(v + int64_t(kvh) * vsh, vst, k0 + 16 * w + c, q_hi, g, va);
  int64_t key[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) key[r] = k0 + 16 * w + 4 * g + r;
  f32x4 acc_k[D / 16], acc_v[D / 16];
#pragma unroll
  for (int t = 0; t < D / 16; ++t) acc_k[t] = acc_v[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  // the local queries that see a key of this block, global: empty for a block before the slice's first sequence (seq_end of its
  // last key <= seq_start[q_off] <= q_off) and for one past the slice (k0 >= q_hi)
  const int64_t q_begin = max64(k0, q_off), q_end = min64(int64_t(seq_end[k1 - 1]), q_hi);
  uint16_t* p_w = p_img + w * 16 * kLdT;
  uint16_t* ds_w = ds_img + w * 16 * kLdT;

  for (int hh = 0; hh < group; ++hh) {
    const int h = kvh * group + hh;
    const uint16_t* qh = q + int64_t(h) * qsh;
    const uint16_t* doh = d_o + int64_t(h) * D;
    for (int64_t q0 = q_begin; q0 < q_end; q0 += kBlk) {
      __syncthreads();
      stage<D, true, true>(qh, qst, q0 - q_off, q_begin - q_off, q_end - q_off, q_rows, q_cols);  // q, dO, lse, delta by local row
      stage<D, true, true>(doh, int64_t(hq) * D, q0 - q_off, q_begin - q_off, q_end - q_off, do_rows, do_cols);
      if (threadIdx.x < kBlk) {
        const int64_t i = q0 + threadIdx.x;
        const bool in = i < q_end;
        lse2_s[threadIdx.x] = in ? lse[int64_t(h) * nq + (i - q_off)] * kLog2e : 0.0f;
        delta_s[threadIdx.x] = in ? delta[int64_t(h) * nq + (i - q_off)] : 0.0f;
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
  // fp32 straight from the accumulators: 16 lanes write the 64 contiguous bytes of a row's 16 columns
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if (key[r] < nk) {
      const int64_t at = (key[r] * hkv + kvh) * D + c;
#pragma unroll
      for (int t = 0; t < D / 16; ++t) {
        dv_part[at + 16 * t] = acc_v[t][r];
        dk_part[at + 16 * t] = acc_k[t][r] * scale;
      }
    }
  }
}

// ---- backward 3: dQ ------------------------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(kThreads) void attn_slice_dq_kernel(const uint16_t* __restrict__ q, int64_t qst, int64_t qsh, const uint16_t* __restrict__ k,
                                                                 int64_t kst, int64_t ksh, const uint16_t* __restrict__ v, int64_t vst, int64_t vsh,
                                                                 float scale, float scale2, const int32_t* __restrict__ seq_start,
                                                                 const float* __restrict__ lse, const float* __restrict__ delta,
                                                                 const uint16_t* __restrict__ d_o, uint16_t* __restrict__ dq, int64_t nq, int64_t q_off,
                                                                 int hq, int group) {
  constexpr int LDD = D + 8;
  __shared__ __attribute__((aligned(16))) uint16_t k_rows[kBlk * LDD];
  __shared__ __attribute__((aligned(16))) uint16_t v_rows[kBlk * LDD];
  __shared__ __attribute__((aligned(16))) uint16_t k_cols[D * kLdT];
  __shared__ __attribute__((aligned(16))) uint16_t ds_img[4 * 16 * kLdT];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int h = blockIdx.y, kvh = h / group;
  const int64_t l0 = int64_t(blockIdx.x) * kBlk, l1 = min64(l0 + kBlk, nq);
  const int64_t q0 = q_off + l0, q1 = q_off + l1;
  const uint16_t* kh = k + int64_t(kvh) * ksh;
  const uint16_t* vh = v + int64_t(kvh) * vsh;
  bf16x8 qa[D / 32], da[D / 32];
  row_frags<D>(q + int64_t(h) * qsh, qst, l0 + 16 * w + c, nq, g, qa);
  row_frags<D>(d_o + int64_t(h) * D, int64_t(hq) * D, l0 + 16 * w + c, nq, g, da);
  int64_t row[4], rs[4];
  float l2[4], dl[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t lrow = l0 + 16 * w + 4 * g + r;
    row[r] = q_off + lrow;
    const bool in = lrow < nq;
    rs[r] = in ? int64_t(seq_start[row[r]]) : (int64_t(1) << 62);
    l2[r] = in ? lse[int64_t(h) * nq + lrow] * kLog2e : 0.0f;
    dl[r] = in ? delta[int64_t(h) * nq + lrow] : 0.0f;
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
  store_tile<D>(acc, sc, k_rows, dq + int64_t(h) * D, int64_t(hq) * D, l0, nq);
}

// ---- fold: out[e] = rne(parts[0][e] + parts[1][e] + ... + parts[P - 1][e]), summed in rank order in fp32 -------------------------
// VEC: 4 elements per thread through 16-byte loads (n_elems a multiple of 4 keeps every part 16-byte aligned); else 1.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void attn_slice_fold_kernel(const float* __restrict__ parts, uint16_t* __restrict__ out, int64_t n_elems, int p) {
  const int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x;
  if constexpr (VEC) {
    const int64_t e = 4 * i;
    if (e >= n_elems) return;
    f32x4 acc = *reinterpret_cast<const f32x4*>(parts + e);
    for (int r = 1; r < p; ++r) {
      const f32x4 x = *reinterpret_cast<const f32x4*>(parts + int64_t(r) * n_elems + e);
      acc = acc + x;
    }
    uint2 packed;
    packed.x = uint32_t(prl_f32_to_bf16_rne(acc[0])) | (uint32_t(prl_f32_to_bf16_rne(acc[1])) << 16);
    packed.y = uint32_t(prl_f32_to_bf16_rne(acc[2])) | (uint32_t(prl_f32_to_bf16_rne(acc[3])) << 16);
    *reinterpret_cast<uint2*>(out + e) = packed;
  } else {
    if (i >= n_elems) return;
    float acc = parts[i];
    for (int r = 1; r < p; ++r) acc = acc + parts[int64_t(r) * n_elems + i];
    out[i] = prl_f32_to_bf16_rne(acc);
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
int check_slice(int64_t nq, int64_t nk, int64_t q_off, int64_t hq, int64_t hkv, int64_t d) {
  PRL_CHECK_ARG(nq >= 0, "negative nq %lld", (long long)nq);
  if (int rc = check_shape(nk, hq, hkv, d)) return rc;
  PRL_CHECK_ARG(q_off >= 0 && nq <= nk && q_off <= nk - nq, "q_off %lld out of range: the %lld local queries must lie inside the %lld keys",
                (long long)q_off, (long long)nq, (long long)nk);
  return PRL_OK;
}

}  // namespace

extern "C" int prl_attn_slice_workspace_bytes(int64_t nq, int64_t hq, size_t* bytes) {
  PRL_CHECK_ARG(bytes != nullptr, "bytes is null");
  PRL_CHECK_ARG(nq >= 0 && nq <= kMaxTokens, "nq %lld is negative or does not fit the int32 segment table", (long long)nq);
  PRL_CHECK_ARG(hq > 0 && hq <= 65535, "hq %lld must be positive and at most 65535", (long long)hq);
  *bytes = workspace_need(nq, hq);
  return PRL_OK;
}

extern "C" int prl_attn_slice_fwd(int64_t nq, int64_t nk, int64_t q_off, int64_t hq, int64_t hkv, int64_t d, const void* q, int64_t q_stride_t,
                                  int64_t q_stride_h, const void* k, int64_t k_stride_t, int64_t k_stride_h, const void* v, int64_t v_stride_t,
                                  int64_t v_stride_h, float scale, const int32_t* seq_start, const int32_t* seq_end, void* out, float* lse,
                                  prl_stream_t stream) {
  if (int rc = check_slice(nq, nk, q_off, hq, hkv, d)) return rc;
  if (nq == 0) return PRL_OK;
  if (int rc = check_operand("q", q, q_stride_t, q_stride_h, d)) return rc;
  if (int rc = check_operand("k", k, k_stride_t, k_stride_h, d)) return rc;
  if (int rc = check_operand("v", v, v_stride_t, v_stride_h, d)) return rc;
  PRL_CHECK_ARG(seq_start != nullptr && seq_end != nullptr && lse != nullptr, "null pointer (seq_start %p, seq_end %p, lse %p)", (const void*)seq_start,
                (const void*)seq_end, (void*)lse);
  PRL_CHECK_ARG(out != nullptr && prl::aligned16(out), "out %p is null or not 16-byte aligned", out);
  const dim3 grid(unsigned(ceil_div(nq, kBlk)), unsigned(hq)), block(kThreads);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const float scale2 = scale * kLog2e;
#define PRL_ATTN_SLICE_FWD(DD)                                                                                                                              \
  hipLaunchKernelGGL(attn_slice_fwd_kernel<DD>, grid, block, 0, st, static_cast<const uint16_t*>(q), q_stride_t, q_stride_h,                                \
                     static_cast<const uint16_t*>(k), k_stride_t, k_stride_h, static_cast<const uint16_t*>(v), v_stride_t, v_stride_h, scale2, seq_start,   \
                     static_cast<uint16_t*>(out), lse, nq, q_off, int(hq), int(hq / hkv))
  if (d == 64) PRL_ATTN_SLICE_FWD(64);
  else PRL_ATTN_SLICE_FWD(128);
#undef PRL_ATTN_SLICE_FWD
  PRL_LAUNCH_CHECK("attn_slice_fwd_kernel");
  return PRL_OK;
}

extern "C" int prl_attn_slice_bwd(int64_t nq, int64_t nk, int64_t q_off, int64_t hq, int64_t hkv, int64_t d, const void* q, int64_t q_stride_t,
                                  int64_t q_stride_h, const void* k, int64_t k_stride_t, int64_t k_stride_h, const void* v, int64_t v_stride_t,
                                  int64_t v_stride_h, float scale, const int32_t* seq_start, const int32_t* seq_end, const void* out, const float* lse,
                                  const void* grad_out, void* grad_q, float* grad_k_part, float* grad_v_part, void* workspace, size_t workspace_bytes,
                                  prl_stream_t stream) {
  if (int rc = check_slice(nq, nk, q_off, hq, hkv, d)) return rc;
  if (nq == 0) return PRL_OK;
  if (int rc = check_operand("q", q, q_stride_t, q_stride_h, d)) return rc;
  if (int rc = check_operand("k", k, k_stride_t, k_stride_h, d)) return rc;
  if (int rc = check_operand("v", v, v_stride_t, v_stride_h, d)) return rc;
  PRL_CHECK_ARG(seq_start != nullptr && seq_end != nullptr && lse != nullptr, "null pointer (seq_start %p, seq_end %p, lse %p)", (const void*)seq_start,
                (const void*)seq_end, (const void*)lse);
  PRL_CHECK_ARG(out != nullptr && grad_out != nullptr && grad_q != nullptr && grad_k_part != nullptr && grad_v_part != nullptr,
                "null pointer (out %p, grad_out %p, grad_q %p, grad_k_part %p, grad_v_part %p)", out, grad_out, grad_q, (void*)grad_k_part,
                (void*)grad_v_part);
  PRL_CHECK_ARG(prl::aligned16(out) && prl::aligned16(grad_out) && prl::aligned16(grad_q) && prl::aligned16(grad_k_part) && prl::aligned16(grad_v_part),
                "out and the gradients must be 16-byte aligned");
  const size_t need = workspace_need(nq, hq);
  PRL_CHECK_ARG(workspace != nullptr && prl::aligned16(workspace), "workspace %p is null or not 16-byte aligned", workspace);
  PRL_CHECK_ARG(workspace_bytes >= need, "workspace too small: %zu < %zu bytes", workspace_bytes, need);
  PRL_CHECK_ARG(ceil_div(nq * hq * (d / 8), kThreads) < (int64_t(1) << 31), "nq %lld x hq %lld rows are too many for one launch", (long long)nq,
                (long long)hq);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const float scale2 = scale * kLog2e;
  float* delta = static_cast<float*>(workspace);
  const int group = int(hq / hkv);
  const dim3 block(kThreads);
  const dim3 grid_delta(unsigned(ceil_div(nq * hq * (d / 8), kThreads)));
  const dim3 grid_kv(unsigned(ceil_div(nk, kBlk)), unsigned(hkv)), grid_q(unsigned(ceil_div(nq, kBlk)), unsigned(hq));
  const uint16_t *qp = static_cast<const uint16_t*>(q), *kp = static_cast<const uint16_t*>(k), *vp = static_cast<const uint16_t*>(v);
  const uint16_t *op = static_cast<const uint16_t*>(out), *gp = static_cast<const uint16_t*>(grad_out);
#define PRL_ATTN_SLICE_BWD(DD)                                                                                                                              \
  do {                                                                                                                                                      \
    hipLaunchKernelGGL(attn_slice_delta_kernel<DD>, grid_delta, block, 0, st, op, gp, delta, nq, int(hq));                                                  \
    PRL_LAUNCH_CHECK("attn_slice_delta_kernel");                                                                                                            \
    hipLaunchKernelGGL(attn_slice_dkv_kernel<DD>, grid_kv, block, 0, st, qp, q_stride_t, q_stride_h, kp, k_stride_t, k_stride_h, vp, v_stride_t,            \
                       v_stride_h, scale, scale2, seq_start, seq_end, lse, delta, gp, grad_k_part, grad_v_part, nq, nk, q_off, int(hq), int(hkv), group);   \
    PRL_LAUNCH_CHECK("attn_slice_dkv_kernel");                                                                                                              \
    hipLaunchKernelGGL(attn_slice_dq_kernel<DD>, grid_q, block, 0, st, qp, q_stride_t, q_stride_h, kp, k_stride_t, k_stride_h, vp, v_stride_t,              \
                       v_stride_h, scale, scale2, seq_start, lse, delta, gp, static_cast<uint16_t*>(grad_q), nq, q_off, int(hq), group);                    \
    PRL_LAUNCH_CHECK("attn_slice_dq_kernel");                                                                                                               \
  } while (0)
  if (d == 64) PRL_ATTN_SLICE_BWD(64);
  else PRL_ATTN_SLICE_BWD(128);
#undef PRL_ATTN_SLICE_BWD
  return PRL_OK;
}

extern "C" int prl_attn_fold_parts(int64_t p, int64_t n_elems, const float* parts, void* out, prl_stream_t stream) {
  PRL_CHECK_ARG(p >= 1 && p <= 65535, "P %lld: at least one part (and at most 65535)", (long long)p);
  PRL_CHECK_ARG(n_elems >= 0, "negative n_elems %lld", (long long)n_elems);
  int64_t total = 0;
  PRL_CHECK_ARG(!__builtin_mul_overflow(p, n_elems, &total) && total < (int64_t(1) << 60), "P %lld x n_elems %lld overflows", (long long)p, (long long)n_elems);
  if (n_elems == 0) return PRL_OK;
  PRL_CHECK_ARG(parts != nullptr && out != nullptr, "null pointer (parts %p, out %p)", (const void*)parts, out);
  PRL_CHECK_ARG(prl::aligned16(parts) && prl::aligned16(out), "parts and out must be 16-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool vec = n_elems % 4 == 0;
  const int64_t blocks = ceil_div(vec ? n_elems / 4 : n_elems, kThreads);
  PRL_CHECK_ARG(blocks < (int64_t(1) << 31), "n_elems %lld is too many for one launch", (long long)n_elems);
  if (vec) hipLaunchKernelGGL(attn_slice_fold_kernel<true>, dim3(unsigned(blocks)), dim3(kThreads), 0, st, parts, static_cast<uint16_t*>(out), n_elems, int(p));
  else hipLaunchKernelGGL(attn_slice_fold_kernel<false>, dim3(unsigned(blocks)), dim3(kThreads), 0, st, parts, static_cast<uint16_t*>(out), n_elems, int(p));
  PRL_LAUNCH_CHECK("attn_slice_fold_kernel");
  return PRL_OK;
}
