// Learner-step boundary: gradient norm + clip coefficient, then the AdamW / Lion update of EVERY parameter,
// as multi-tensor launches (one per <= 64 gradients for the norm, per <= 32 parameters for the step); and, in front of it, the
// fold of every micro-batch's gradients into fp32 accumulators (one launch per <= 64 gradients), one rank's or every rank's copy at once.
//
// Replaces `torch.nn.utils.clip_grad_norm_` -> `float(gn)` -> `optimizer.step()` of
// pipelinerl/finetune_loop.py:738-744 (a multi-pass foreach norm, a host sync, an in-place rescale of every
// gradient, then the optimizer's own passes) and the `Lion` / `AdamW` of pipelinerl/finetune/optim.py:25-112.
//
// HBM-bound streaming in the shape of prl_copy.hip: the segment table travels in the kernel arguments, a
// workgroup owns one 16 Ki-element chunk found by scalar binary search, a lane moves 8 consecutive elements per
// iteration with 16-byte loads and stores (up to 8 independent loads in flight per lane and iteration).
// Algorithmic bytes per element, bf16 parameter + bf16 gradient + fp32 master: AdamW 2+4+4+4 read, 4+4+4+2
// written = 28; Lion 20; the norm pass 2 (bf16) or 4 (fp32).
//
// The norm is reduced without atomics in a fixed order (fp64 per lane -> wave shuffle tree -> waves in order ->
// one record per chunk -> a one-workgroup finalize), so two runs give the same bits; the clip coefficient
// stays on the device and the step kernels read it from there: no host synchronisation on the boundary.
#include "prl_common.h"
#include "prl_optim_io.h"
#include "prl_optim_math.h"

namespace {

using prl::kWave;
using namespace prl::optim_io;  // load8 / store8 / load1 / store1 / owner, kGroup = 8 elements per lane and iteration

constexpr int kBlock = 256;
constexpr int64_t kChunk = 16 << 10;       // elements per workgroup: 8 iterations of 256 lanes x 8 elements
constexpr int kNormSegs = 64;              // per launch: 64 x 21 B of kernel arguments
constexpr int kAccumSegs = 64;             // per launch: 64 x 29 B (both fold kernels)
constexpr int kStepSegs = 32;              // per launch: 32 x 90 B (64 would not fit 4 KB of kernel arguments)
constexpr int kFinalBlock = 1024;

// ---- gradient norm --------------------------------------------------------------------------------------------------
struct NormTable {
  const void* grad[kNormSegs];
  int64_t numel[kNormSegs];
  int32_t first_chunk[kNormSegs + 1];
  uint8_t bf16[kNormSegs];
  int32_t n;
  int32_t partial_base;  // index of this launch's first chunk in the partial array
};

template <bool BF16>
__device__ __forceinline__ double chunk_sumsq(const void* g, int64_t len) {
  double acc = 0.0;
  int64_t done = 0;
  if (aligned16_dev(g)) {
    const int64_t ngroups = len / kGroup;
    for (int64_t q = threadIdx.x; q < ngroups; q += kBlock) {
      float x[kGroup];
      load8<BF16>(g, q * kGroup, x);
#pragma unroll
      for (int k = 0; k < kGroup; ++k) {
        const double d = (double)x[k];
        acc += d * d;  // the square of an fp32 value is exact in fp64
      }
    }
    done = ngroups * kGroup;
  }
  for (int64_t i = done + threadIdx.x; i < len; i += kBlock) {  // tail, or a whole unaligned view
    const double d = (double)load1<BF16>(g, i);
    acc += d * d;
  }
  return acc;
}

__global__ __launch_bounds__(kBlock) void grad_sumsq_kernel(const NormTable tab, double* __restrict__ partials) {
  __shared__ double red[kBlock / kWave];
  const int chunk = blockIdx.x;
  const int s = owner(tab.first_chunk, tab.n, chunk);
  const int64_t begin = int64_t(chunk - tab.first_chunk[s]) * kChunk;
  const int64_t left = tab.numel[s] - begin;
  const int64_t len = left < kChunk ? left : kChunk;
  double acc;
  if (tab.bf16[s]) acc = chunk_sumsq<true>(static_cast<const uint16_t*>(tab.grad[s]) + begin, len);
  else acc = chunk_sumsq<false>(static_cast<const float*>(tab.grad[s]) + begin, len);
  acc = prl::wave_sum(acc);
  if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = red[0];
#pragma unroll
    for (int w = 1; w < kBlock / kWave; ++w) t += red[w];
    partials[tab.partial_base + chunk] = t;
  }
}

// One workgroup folds the per-chunk records in a fixed order: thread t takes records t, t + 1024, ... into four
// independent accumulators (the loads overlap), then the 1024 per-thread sums are added in index order by a tree.
// Every thread returns; thread 0's value is the sum.
__device__ __forceinline__ double fold_partials(const double* __restrict__ partials, int64_t n, double (&lds)[kFinalBlock]) {
  double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0;
  int64_t i = threadIdx.x;
  for (; i + 3 * kFinalBlock < n; i += 4 * kFinalBlock) {
    v0 += partials[i];
    v1 += partials[i + kFinalBlock];
    v2 += partials[i + 2 * kFinalBlock];
    v3 += partials[i + 3 * kFinalBlock];
  }
  for (; i < n; i += kFinalBlock) v0 += partials[i];
  lds[threadIdx.x] = (v0 + v1) + (v2 + v3);
  __syncthreads();
  for (int stride = kFinalBlock / 2; stride > 0; stride >>= 1) {
    if ((int)threadIdx.x < stride) lds[threadIdx.x] += lds[threadIdx.x + stride];
    __syncthreads();
  }
  return lds[0];
}

__device__ __forceinline__ void write_norm_record(double sumsq, float max_norm, float* __restrict__ norm_and_coef) {
  const float norm = (float)sqrt(sumsq);
  norm_and_coef[0] = norm;
  norm_and_coef[1] = prl_clip_coef(norm, max_norm);
}

__global__ __launch_bounds__(kFinalBlock) void grad_norm_finalize_kernel(const double* __restrict__ partials, int64_t n, float max_norm,
                                                                         float* __restrict__ norm_and_coef) {
  __shared__ double lds[kFinalBlock];
  const double sumsq = fold_partials(partials, n, lds);
  if (threadIdx.x == 0) write_norm_record(sumsq, max_norm, norm_and_coef);
}

// The two halves of the finalize for a norm that crosses ranks: the fold leaves the fp64 sum of squares of THIS rank's
// segments on the device, the ranks add theirs, the record is formed from the total.
__global__ __launch_bounds__(kFinalBlock) void grad_sumsq_fold_kernel(const double* __restrict__ partials, int64_t n, double* __restrict__ sumsq) {
  __shared__ double lds[kFinalBlock];
  const double t = fold_partials(partials, n, lds);
  if (threadIdx.x == 0) *sumsq = t;
}

__global__ void clip_from_sumsq_kernel(const double* __restrict__ sumsq, float max_norm, float* __restrict__ norm_and_coef) {
  if (blockIdx.x == 0 && threadIdx.x == 0) write_norm_record(*sumsq, max_norm, norm_and_coef);
}

// ---- the step ---------------------------------------------------------------------------------------------------------
struct AdamwRule {
  using Scalars = PrlAdamwScalars;
  static constexpr bool kSecondMoment = true;
};
struct LionRule {
  using Scalars = PrlLionScalars;
  static constexpr bool kSecondMoment = false;
};

template <class Rule>
struct StepTable {
  void* param[kStepSegs];
  const void* grad[kStepSegs];
  float* master[kStepSegs];  // null: the parameter itself carries the weights
  float* exp_avg[kStepSegs];
  float* exp_avg_sq[kStepSegs];
  int64_t numel[kStepSegs];
  typename Rule::Scalars sc[kStepSegs];
  int32_t first_chunk[kStepSegs + 1];
  uint8_t param_bf16[kStepSegs];
  uint8_t grad_bf16[kStepSegs];
  int32_t n;
};

__device__ __forceinline__ void apply(const PrlAdamwScalars& s, float coef, float g, float& p, float& m, float& v) { prl_adamw_update(s, coef, g, p, m, v); }
__device__ __forceinline__ void apply(const PrlLionScalars& s, float coef, float g, float& p, float& m, float& v) { prl_lion_update(s, coef, g, p, m); }

// One chunk.  PB / GB: bf16 parameter / gradient; MW: fp32 master weights (the bf16 parameter is only written).
template <class Rule, bool PB, bool GB, bool MW>
__device__ __forceinline__ void chunk_step(const typename Rule::Scalars sc, float coef, void* param, const void* grad, float* master, float* m_ptr,
                                           float* v_ptr, int64_t len) {
  constexpr bool V = Rule::kSecondMoment;
  constexpr bool WB = MW ? false : PB;  // dtype of the array the weights are READ from
  const void* w_src = MW ? static_cast<const void*>(master) : static_cast<const void*>(param);
  int64_t done = 0;
  const bool vec_ok = aligned16_dev(param) && aligned16_dev(grad) && aligned16_dev(m_ptr) && (!V || aligned16_dev(v_ptr)) && (!MW || aligned16_dev(master));
  if (vec_ok) {
    const int64_t ngroups = len / kGroup;
    for (int64_t q = threadIdx.x; q < ngroups; q += kBlock) {
      const int64_t i = q * kGroup;
      float g[kGroup], w[kGroup], m[kGroup], v[kGroup];
      load8<GB>(grad, i, g);
      load8<WB>(w_src, i, w);
      load8<false>(m_ptr, i, m);
      if constexpr (V) load8<false>(v_ptr, i, v);
#pragma unroll
      for (int k = 0; k < kGroup; ++k) apply(sc, coef, g[k], w[k], m[k], v[k]);
      store8_stream(m_ptr, i, m);
      if constexpr (V) store8_stream(v_ptr, i, v);
      if constexpr (MW) store8_stream(master, i, w);
      store8<PB>(param, i, w);
    }
    done = ngroups * kGroup;
  }
  for (int64_t i = done + threadIdx.x; i < len; i += kBlock) {  // tail, or a whole unaligned view
    float w = load1<WB>(w_src, i), m = m_ptr[i], v = 0.0f;
    if constexpr (V) v = v_ptr[i];
    apply(sc, coef, load1<GB>(grad, i), w, m, v);
    m_ptr[i] = m;
    if constexpr (V) v_ptr[i] = v;
    if constexpr (MW) master[i] = w;
    store1<PB>(param, i, w);
  }
}

template <class Rule>
__global__ __launch_bounds__(kBlock) void optim_step_kernel(const StepTable<Rule> tab, const float* __restrict__ norm_and_coef) {
  const int chunk = blockIdx.x;
  const int s = owner(tab.first_chunk, tab.n, chunk);
  const int64_t begin = int64_t(chunk - tab.first_chunk[s]) * kChunk;
  const int64_t left = tab.numel[s] - begin;
  const int64_t len = left < kChunk ? left : kChunk;
  const float coef = norm_and_coef ? norm_and_coef[1] : 1.0f;
  const bool pb = tab.param_bf16[s], gb = tab.grad_bf16[s];
  const int64_t pe = pb ? 2 : 4, ge = gb ? 2 : 4;
  void* param = static_cast<char*>(tab.param[s]) + begin * pe;
  const void* grad = static_cast<const char*>(tab.grad[s]) + begin * ge;
  float* master = tab.master[s] ? tab.master[s] + begin : nullptr;
  float* m = tab.exp_avg[s] + begin;
  float* v = Rule::kSecondMoment ? tab.exp_avg_sq[s] + begin : nullptr;
  const typename Rule::Scalars sc = tab.sc[s];
  // wave-uniform dispatch on the segment's dtypes (a master exists for bf16 parameters only)
  if (!pb) {
    if (gb) chunk_step<Rule, false, true, false>(sc, coef, param, grad, nullptr, m, v, len);
    else chunk_step<Rule, false, false, false>(sc, coef, param, grad, nullptr, m, v, len);
  } else if (master) {
    if (gb) chunk_step<Rule, true, true, true>(sc, coef, param, grad, master, m, v, len);
    else chunk_step<Rule, true, false, true>(sc, coef, param, grad, master, m, v, len);
  } else {
    if (gb) chunk_step<Rule, true, true, false>(sc, coef, param, grad, nullptr, m, v, len);
    else chunk_step<Rule, true, false, false>(sc, coef, param, grad, nullptr, m, v, len);
  }
}

// ---- gradient accumulation ---------------------------------------------------------------------------------------------
// acc (fp32) = [acc +] (float)grad, one micro-batch.  10 B/element for a bf16 gradient (2 + 4 read, 4 written), 6 on the overwriting
// first fold of a step (the accumulator is not read: no zeroing pass exists), 12 / 8 for an fp32 gradient.  Every element is owned by
// one lane: no atomics, and the sum over the micro-batches is the sequential fp32 sum in fold order.
struct AccumTable {
  const void* grad[kAccumSegs];
  float* acc[kAccumSegs];
  int64_t numel[kAccumSegs];
  int32_t first_chunk[kAccumSegs + 1];
  uint8_t bf16[kAccumSegs];
  int32_t n;
};

template <bool GB, bool OVERWRITE>
__device__ __forceinline__ void chunk_accumulate(const void* grad, float* acc, int64_t len) {
  int64_t done = 0;
  if (aligned16_dev(grad) && aligned16_dev(acc)) {
    const int64_t ngroups = len / kGroup;
    for (int64_t q = threadIdx.x; q < ngroups; q += kBlock) {
      const int64_t i = q * kGroup;
      float g[kGroup], a[kGroup];
      load8<GB>(grad, i, g);
      if constexpr (!OVERWRITE) load8<false>(acc, i, a);
#pragma unroll
      for (int k = 0; k < kGroup; ++k) a[k] = OVERWRITE ? prl_grad_accum_first(g[k]) : prl_grad_accum_add(a[k], g[k]);
      store8_stream(acc, i, a);  // read next by the following fold, a whole backward later
    }
    done = ngroups * kGroup;
  }
  for (int64_t i = done + threadIdx.x; i < len; i += kBlock) {  // tail, or a whole unaligned view
    const float g = load1<GB>(grad, i);
    acc[i] = OVERWRITE ? prl_grad_accum_first(g) : prl_grad_accum_add(acc[i], g);
  }
}

template <bool OVERWRITE>
__global__ __launch_bounds__(kBlock) void grad_accumulate_kernel(const AccumTable tab) {
  const int chunk = blockIdx.x;
  const int s = owner(tab.first_chunk, tab.n, chunk);
  const int64_t begin = int64_t(chunk - tab.first_chunk[s]) * kChunk;
  const int64_t left = tab.numel[s] - begin;
  const int64_t len = left < kChunk ? left : kChunk;
  float* acc = tab.acc[s] + begin;
  if (tab.bf16[s]) chunk_accumulate<true, OVERWRITE>(static_cast<const uint16_t*>(tab.grad[s]) + begin, acc, len);
  else chunk_accumulate<false, OVERWRITE>(static_cast<const float*>(tab.grad[s]) + begin, acc, len);
}

// The same fold over the `world` ranks' copies of one piece at once (sharded gradients: what an all-to-all delivered): rank r's copy
// stands `stride` bytes behind rank r - 1's.  acc = (((acc + g_0) + g_1) + ...) + g_{world-1}, the adds in rank order, so the result is
// what `world` calls of the kernel above give, bit for bit - for 8 + world x itemsize bytes per element instead of world x (8 + itemsize).
// Four ranks' loads are issued before their adds (a remainder loop takes world mod 4); `stride` is a multiple of 16, so every rank's
// copy has the alignment of rank 0's.
struct AccumRanksTable {
  const void* src[kAccumSegs];
  float* acc[kAccumSegs];
  int64_t numel[kAccumSegs];
  int32_t first_chunk[kAccumSegs + 1];
  uint8_t bf16[kAccumSegs];
  int32_t n;
  int32_t world;
  int64_t stride;  // bytes between two ranks' copies
};

__device__ __forceinline__ const void* rank_copy(const void* src, int64_t stride, int r) { return static_cast<const char*>(src) + int64_t(r) * stride; }

template <bool GB, bool OVERWRITE>
__device__ __forceinline__ void chunk_accumulate_ranks(const void* src, int64_t stride, int world, float* acc, int64_t len) {
  int64_t done = 0;
  if (aligned16_dev(src) && aligned16_dev(acc)) {
    const int64_t ngroups = len / kGroup;
    for (int64_t q = threadIdx.x; q < ngroups; q += kBlock) {
      const int64_t i = q * kGroup;
      float a[kGroup];
      int r = 0;
      if constexpr (OVERWRITE) {
        float g[kGroup];
        load8<GB>(src, i, g);
#pragma unroll
        for (int k = 0; k < kGroup; ++k) a[k] = prl_grad_accum_first(g[k]);
        r = 1;
      } else {
        load8<false>(acc, i, a);
      }
      for (; r + 4 <= world; r += 4) {
        float g0[kGroup], g1[kGroup], g2[kGroup], g3[kGroup];
        load8<GB>(rank_copy(src, stride, r), i, g0);
        load8<GB>(rank_copy(src, stride, r + 1), i, g1);
        load8<GB>(rank_copy(src, stride, r + 2), i, g2);
        load8<GB>(rank_copy(src, stride, r + 3), i, g3);
#pragma unroll
        for (int k = 0; k < kGroup; ++k)
          a[k] = prl_grad_accum_add(prl_grad_accum_add(prl_grad_accum_add(prl_grad_accum_add(a[k], g0[k]), g1[k]), g2[k]), g3[k]);
      }
      for (; r < world; ++r) {
        float g[kGroup];
        load8<GB>(rank_copy(src, stride, r), i, g);
#pragma unroll
        for (int k = 0; k < kGroup; ++k) a[k] = prl_grad_accum_add(a[k], g[k]);
      }
      store8_stream(acc, i, a);  // read next by the following fold, a whole backward later
    }
    done = ngroups * kGroup;
  }
  for (int64_t i = done + threadIdx.x; i < len; i += kBlock) {  // tail, or a whole unaligned view
    float a = OVERWRITE ? prl_grad_accum_first(load1<GB>(src, i)) : acc[i];
    for (int r = OVERWRITE ? 1 : 0; r < world; ++r) a = prl_grad_accum_add(a, load1<GB>(rank_copy(src, stride, r), i));
    acc[i] = a;
  }
}

template <bool OVERWRITE>
__global__ __launch_bounds__(kBlock) void grad_accumulate_ranks_kernel(const AccumRanksTable tab) {
  const int chunk = blockIdx.x;
  const int s = owner(tab.first_chunk, tab.n, chunk);
  const int64_t begin = int64_t(chunk - tab.first_chunk[s]) * kChunk;
  const int64_t left = tab.numel[s] - begin;
  const int64_t len = left < kChunk ? left : kChunk;
  float* acc = tab.acc[s] + begin;
  if (tab.bf16[s]) chunk_accumulate_ranks<true, OVERWRITE>(static_cast<const uint16_t*>(tab.src[s]) + begin, tab.stride, tab.world, acc, len);
  else chunk_accumulate_ranks<false, OVERWRITE>(static_cast<const float*>(tab.src[s]) + begin, tab.stride, tab.world, acc, len);
}

int64_t chunks_of(int64_t numel) { return (numel + kChunk - 1) / kChunk; }
bool live(const prl_optim_segment& s) { return s.grad != nullptr && s.numel > 0; }

int validate(const prl_optim_segment* segs, int64_t n, bool need_state, bool need_second) {
  PRL_CHECK_ARG(n >= 0, "negative segment count");
  PRL_CHECK_ARG(n == 0 || segs != nullptr, "null segment table with %lld segments", (long long)n);
  for (int64_t i = 0; i < n; ++i) {
    const prl_optim_segment& s = segs[i];
    PRL_CHECK_ARG(s.numel >= 0, "segment %lld: negative numel %lld", (long long)i, (long long)s.numel);
    PRL_CHECK_ARG(chunks_of(s.numel) < (int64_t(1) << 30), "segment %lld: %lld elements are too many for one launch", (long long)i, (long long)s.numel);
    PRL_CHECK_ARG(s.grad_dtype == PRL_DTYPE_F32 || s.grad_dtype == PRL_DTYPE_BF16, "segment %lld: unknown grad_dtype %d", (long long)i, s.grad_dtype);
    PRL_CHECK_ARG(s.param_dtype == PRL_DTYPE_F32 || s.param_dtype == PRL_DTYPE_BF16, "segment %lld: unknown param_dtype %d", (long long)i, s.param_dtype);
    if (!need_state || !live(s)) continue;
    PRL_CHECK_ARG(s.param != nullptr && s.exp_avg != nullptr, "segment %lld: null param or exp_avg", (long long)i);
    PRL_CHECK_ARG(!need_second || s.exp_avg_sq != nullptr, "segment %lld: null exp_avg_sq", (long long)i);
    PRL_CHECK_ARG(s.master == nullptr || s.param_dtype == PRL_DTYPE_BF16, "segment %lld: master weights go with a bf16 parameter", (long long)i);
    PRL_CHECK_ARG(s.step >= 1, "segment %lld: step %lld (the number of this update) must be >= 1", (long long)i, (long long)s.step);
  }
  return PRL_OK;
}

void fill_scalars(PrlAdamwScalars& o, const prl_optim_segment& s, double beta1, double beta2, double eps) { o = prl_adamw_scalars(s.lr, s.weight_decay, beta1, beta2, eps, s.step); }
void fill_scalars(PrlLionScalars& o, const prl_optim_segment& s, double beta1, double beta2, double) { o = prl_lion_scalars(s.lr, s.weight_decay, beta1, beta2); }

template <class Rule>
int step_launches(const prl_optim_segment* segs, int64_t n, double beta1, double beta2, double eps, const float* norm_and_coef, hipStream_t stream) {
  int64_t i = 0;
  while (i < n) {
    StepTable<Rule> tab;
    tab.n = 0;
    tab.first_chunk[0] = 0;
    int64_t chunks = 0;
    for (; i < n && tab.n < kStepSegs; ++i) {
      const prl_optim_segment& s = segs[i];
      if (!live(s)) continue;
      const int64_t c = chunks_of(s.numel);
      if (chunks + c > (int64_t(1) << 30)) break;  // keep the grid and the prefix sums in int32
      const int k = tab.n;
      tab.param[k] = s.param;
      tab.grad[k] = s.grad;
      tab.master[k] = static_cast<float*>(s.master);
      tab.exp_avg[k] = static_cast<float*>(s.exp_avg);
      tab.exp_avg_sq[k] = static_cast<float*>(s.exp_avg_sq);
      tab.numel[k] = s.numel;
      tab.param_bf16[k] = s.param_dtype == PRL_DTYPE_BF16;
      tab.grad_bf16[k] = s.grad_dtype == PRL_DTYPE_BF16;
      fill_scalars(tab.sc[k], s, beta1, beta2, eps);
      chunks += c;
      tab.first_chunk[++tab.n] = int32_t(chunks);
    }
    if (tab.n == 0) break;  // only skipped segments were left (validate() bounds every single segment)
    hipLaunchKernelGGL(optim_step_kernel<Rule>, dim3(unsigned(chunks)), dim3(kBlock), 0, stream, tab, norm_and_coef);
    PRL_LAUNCH_CHECK("optim_step_kernel");
  }
  return PRL_OK;
}

}  // namespace

extern "C" int prl_optim_workspace_bytes(int64_t n_segments, int64_t total_numel, size_t* bytes) {
  PRL_CHECK_ARG(bytes != nullptr, "bytes is null");
  PRL_CHECK_ARG(n_segments >= 0 && total_numel >= 0, "negative size");
  // one fp64 record per chunk; every segment may end in a partial chunk
  *bytes = (size_t)(total_numel / kChunk + n_segments + 1) * sizeof(double);
  return PRL_OK;
}

// (the caller has validated the table) one grad_sumsq_kernel launch per <= 64 live segments; *n_partials = number of per-chunk records written
static int launch_partials(const prl_optim_segment* segments, int64_t n_segments, void* workspace, size_t workspace_bytes, hipStream_t s,
                           int64_t* n_partials) {
  int64_t total_chunks = 0;
  for (int64_t i = 0; i < n_segments; ++i)
    if (live(segments[i])) total_chunks += chunks_of(segments[i].numel);
  PRL_CHECK_ARG(total_chunks < (int64_t(1) << 31), "%lld chunks do not fit the partial index", (long long)total_chunks);
  PRL_CHECK_ARG(total_chunks == 0 || workspace != nullptr, "workspace is null");
  PRL_CHECK_ARG(workspace_bytes >= (size_t)total_chunks * sizeof(double), "workspace too small: %zu < %zu bytes for %lld chunks", workspace_bytes,
                (size_t)total_chunks * sizeof(double), (long long)total_chunks);
  double* partials = static_cast<double*>(workspace);
  int64_t i = 0, base = 0;
  while (i < n_segments) {
    NormTable tab;
    tab.n = 0;
    tab.first_chunk[0] = 0;
    tab.partial_base = int32_t(base);
    int64_t chunks = 0;
    for (; i < n_segments && tab.n < kNormSegs; ++i) {
      const prl_optim_segment& g = segments[i];
      if (!live(g)) continue;
      const int64_t c = chunks_of(g.numel);
      if (chunks + c > (int64_t(1) << 30)) break;
      tab.grad[tab.n] = g.grad;
      tab.numel[tab.n] = g.numel;
      tab.bf16[tab.n] = g.grad_dtype == PRL_DTYPE_BF16;
      chunks += c;
      tab.first_chunk[++tab.n] = int32_t(chunks);
    }
    if (tab.n == 0) break;
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(unsigned(chunks)), dim3(kBlock), 0, s, tab, partials);
    PRL_LAUNCH_CHECK("grad_sumsq_kernel");
    base += chunks;
  }
  *n_partials = base;
  return PRL_OK;
}

extern "C" int prl_optim_grad_norm(const prl_optim_segment* segments, int64_t n_segments, float max_norm, void* workspace,
                                   size_t workspace_bytes, float* norm_and_coef, prl_stream_t stream) {
  if (int rc = validate(segments, n_segments, false, false)) return rc;
  PRL_CHECK_ARG(norm_and_coef != nullptr, "norm_and_coef is null");
  hipStream_t s = static_cast<hipStream_t>(stream);
  int64_t base = 0;
  if (int rc = launch_partials(segments, n_segments, workspace, workspace_bytes, s, &base)) return rc;
  hipLaunchKernelGGL(grad_norm_finalize_kernel, dim3(1), dim3(kFinalBlock), 0, s, static_cast<const double*>(workspace), base, max_norm, norm_and_coef);
  PRL_LAUNCH_CHECK("grad_norm_finalize_kernel");
  return PRL_OK;
}

extern "C" int prl_optim_grad_sumsq(const prl_optim_segment* segments, int64_t n_segments, void* workspace, size_t workspace_bytes,
                                    double* sumsq, prl_stream_t stream) {
  if (int rc = validate(segments, n_segments, false, false)) return rc;
  PRL_CHECK_ARG(sumsq != nullptr, "sumsq is null");
  hipStream_t s = static_cast<hipStream_t>(stream);
  int64_t base = 0;
  if (int rc = launch_partials(segments, n_segments, workspace, workspace_bytes, s, &base)) return rc;
  hipLaunchKernelGGL(grad_sumsq_fold_kernel, dim3(1), dim3(kFinalBlock), 0, s, static_cast<const double*>(workspace), base, sumsq);  // no segment: writes 0
  PRL_LAUNCH_CHECK("grad_sumsq_fold_kernel");
  return PRL_OK;
}

extern "C" int prl_optim_clip_from_sumsq(const double* sumsq, float max_norm, float* norm_and_coef, prl_stream_t stream) {
  PRL_CHECK_ARG(sumsq != nullptr, "sumsq is null");
  PRL_CHECK_ARG(norm_and_coef != nullptr, "norm_and_coef is null");
  hipLaunchKernelGGL(clip_from_sumsq_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), sumsq, max_norm, norm_and_coef);
  PRL_LAUNCH_CHECK("clip_from_sumsq_kernel");
  return PRL_OK;
}

extern "C" int prl_optim_adamw_step(const prl_optim_segment* segments, int64_t n_segments, double beta1, double beta2, double eps,
                                    const float* norm_and_coef, prl_stream_t stream) {
  if (int rc = validate(segments, n_segments, true, true)) return rc;
  PRL_CHECK_ARG(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "betas (%g, %g) outside [0, 1)", beta1, beta2);
  PRL_CHECK_ARG(eps >= 0.0, "negative eps %g", eps);
  return step_launches<AdamwRule>(segments, n_segments, beta1, beta2, eps, norm_and_coef, static_cast<hipStream_t>(stream));
}

extern "C" int prl_optim_lion_step(const prl_optim_segment* segments, int64_t n_segments, double beta1, double beta2,
                                   const float* norm_and_coef, prl_stream_t stream) {
  if (int rc = validate(segments, n_segments, true, false)) return rc;
  PRL_CHECK_ARG(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "betas (%g, %g) outside [0, 1)", beta1, beta2);
  return step_launches<LionRule>(segments, n_segments, beta1, beta2, 0.0, norm_and_coef, static_cast<hipStream_t>(stream));
}

extern "C" int prl_optim_grad_accumulate(const prl_accum_segment* segments, int64_t n_segments, int32_t overwrite, prl_stream_t stream) {
  PRL_CHECK_ARG(n_segments >= 0, "negative segment count");
  PRL_CHECK_ARG(n_segments == 0 || segments != nullptr, "null segment table with %lld segments", (long long)n_segments);
  for (int64_t i = 0; i < n_segments; ++i) {
    const prl_accum_segment& s = segments[i];
    PRL_CHECK_ARG(s.numel >= 0, "segment %lld: negative numel %lld", (long long)i, (long long)s.numel);
    PRL_CHECK_ARG(chunks_of(s.numel) < (int64_t(1) << 30), "segment %lld: %lld elements are too many for one launch", (long long)i, (long long)s.numel);
    PRL_CHECK_ARG(s.grad_dtype == PRL_DTYPE_F32 || s.grad_dtype == PRL_DTYPE_BF16, "segment %lld: unknown grad_dtype %d", (long long)i, s.grad_dtype);
    PRL_CHECK_ARG(s.grad == nullptr || s.numel == 0 || s.acc != nullptr, "segment %lld: null acc", (long long)i);
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  int64_t i = 0;
  while (i < n_segments) {
    AccumTable tab;
    tab.n = 0;
    tab.first_chunk[0] = 0;
    int64_t chunks = 0;
    for (; i < n_segments && tab.n < kAccumSegs; ++i) {
      const prl_accum_segment& s = segments[i];
      if (s.grad == nullptr || s.numel == 0) continue;
      const int64_t c = chunks_of(s.numel);
      if (chunks + c > (int64_t(1) << 30)) break;  // keep the grid and the prefix sums in int32
      tab.grad[tab.n] = s.grad;
      tab.acc[tab.n] = static_cast<float*>(s.acc);
      tab.numel[tab.n] = s.numel;
      tab.bf16[tab.n] = s.grad_dtype == PRL_DTYPE_BF16;
      chunks += c;
      tab.first_chunk[++tab.n] = int32_t(chunks);
    }
    if (tab.n == 0) break;  // only skipped segments were left
    if (overwrite) hipLaunchKernelGGL(grad_accumulate_kernel<true>, dim3(unsigned(chunks)), dim3(kBlock), 0, st, tab);
    else hipLaunchKernelGGL(grad_accumulate_kernel<false>, dim3(unsigned(chunks)), dim3(kBlock), 0, st, tab);
    PRL_LAUNCH_CHECK("grad_accumulate_kernel");
  }
  return PRL_OK;
}

extern "C" int prl_optim_grad_accumulate_ranks(const prl_accum_ranks_segment* segments, int64_t n_segments, int32_t world,
                                               int64_t rank_stride_bytes, int32_t overwrite, prl_stream_t stream) {
  PRL_CHECK_ARG(n_segments >= 0, "negative segment count");
  PRL_CHECK_ARG(n_segments == 0 || segments != nullptr, "null segment table with %lld segments", (long long)n_segments);
  PRL_CHECK_ARG(world >= 1 && world <= PRL_ACCUM_RANKS_MAX_WORLD, "world %d outside [1, %d]", world, PRL_ACCUM_RANKS_MAX_WORLD);
  PRL_CHECK_ARG(rank_stride_bytes >= 0 && rank_stride_bytes % 16 == 0, "rank_stride_bytes %lld is negative or not a multiple of 16",
                (long long)rank_stride_bytes);
  for (int64_t i = 0; i < n_segments; ++i) {
    const prl_accum_ranks_segment& s = segments[i];
    PRL_CHECK_ARG(s.numel >= 0, "segment %lld: negative numel %lld", (long long)i, (long long)s.numel);
    PRL_CHECK_ARG(chunks_of(s.numel) < (int64_t(1) << 30), "segment %lld: %lld elements are too many for one launch", (long long)i, (long long)s.numel);
    PRL_CHECK_ARG(s.src_dtype == PRL_DTYPE_F32 || s.src_dtype == PRL_DTYPE_BF16, "segment %lld: unknown src_dtype %d", (long long)i, s.src_dtype);
    PRL_CHECK_ARG(s.src == nullptr || s.numel == 0 || s.acc != nullptr, "segment %lld: null acc", (long long)i);
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  int64_t i = 0;
  while (i < n_segments) {
    AccumRanksTable tab;
    tab.n = 0;
    tab.world = world;
    tab.stride = rank_stride_bytes;
    tab.first_chunk[0] = 0;
    int64_t chunks = 0;
    for (; i < n_segments && tab.n < kAccumSegs; ++i) {
      const prl_accum_ranks_segment& s = segments[i];
      if (s.src == nullptr || s.numel == 0) continue;
      const int64_t c = chunks_of(s.numel);
      if (chunks + c > (int64_t(1) << 30)) break;  // keep the grid and the prefix sums in int32
      tab.src[tab.n] = s.src;
      tab.acc[tab.n] = static_cast<float*>(s.acc);
      tab.numel[tab.n] = s.numel;
      tab.bf16[tab.n] = s.src_dtype == PRL_DTYPE_BF16;
      chunks += c;
      tab.first_chunk[++tab.n] = int32_t(chunks);
    }
    if (tab.n == 0) break;  // only skipped segments were left
    if (overwrite) hipLaunchKernelGGL(grad_accumulate_ranks_kernel<true>, dim3(unsigned(chunks)), dim3(kBlock), 0, st, tab);
    else hipLaunchKernelGGL(grad_accumulate_ranks_kernel<false>, dim3(unsigned(chunks)), dim3(kBlock), 0, st, tab);
    PRL_LAUNCH_CHECK("grad_accumulate_ranks_kernel");
  }
  return PRL_OK;
}
