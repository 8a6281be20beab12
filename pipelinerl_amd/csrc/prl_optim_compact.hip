// The AdamW / Lion step of prl_optim.hip with compact state: `exp_avg` / `exp_avg_sq` kept in bf16, and / or a bf16 parameter
// without a master copy, every bf16 store of a value that is "the truth" rounded STOCHASTICALLY (prl_optim_sr.h) so that
// updates below half an ulp survive in expectation.  The per-element arithmetic is prl_adamw_update / prl_lion_update unchanged:
// widen (exact), update in fp32, round the stores.  Only loads and stores differ from optim_step_kernel.
//
// Same shape as optim_step_kernel: the segment table travels in the kernel arguments (<= 32 segments per launch), a workgroup owns
// one 16 Ki-element chunk found by scalar binary search, a lane moves 8 consecutive elements per iteration with 16-byte accesses
// (8 bf16 per access for compact state), tails and unaligned views take a scalar path, the dispatch on dtypes is wave-uniform.
// Algorithmic bytes per element, bf16 parameter + bf16 gradient, no master, bf16 state: AdamW 2+2+2+2 read, 2+2+2 written = 14
// (28 with fp32 state and master); Lion 10 (20).
//
// Random bits: two Philox4x32-10 calls per 8-element group (80 32-bit multiplies), keyed on the seed and counted by the element's
// index inside its PARAMETER (elem_offset + index in the piece), the step and the parameter's ordinal - so a sharded run rounds
// every element as the unsharded one does.  Segments that store nothing stochastically (fp32 state and a parameter written
// exactly or to nearest) make no call.
#include "prl_common.h"
#include "prl_optim_io.h"
#include "prl_optim_math.h"
#include "prl_optim_sr.h"

namespace {

using namespace prl::optim_io;  // load8 / store8 / load1 / store1 / owner, kGroup = 8 elements per lane and iteration

constexpr int kBlock = 256;
constexpr int64_t kChunk = 16 << 10;  // elements per workgroup, as in prl_optim.hip
constexpr int kStepSegs = 32;         // per launch: 32 x 108 B

struct AdamwRule {
  using Scalars = PrlAdamwScalars;
  static constexpr bool kSecondMoment = true;
};
struct LionRule {
  using Scalars = PrlLionScalars;
  static constexpr bool kSecondMoment = false;
};

// how the weights are read and written
enum ParamMode : int {
  kParamF32 = 0,       // fp32 parameter, written exactly
  kParamMaster = 1,    // bf16 parameter = RNE image of the fp32 master, which is read and written
  kParamNearest = 2,   // bf16 parameter read, written to nearest even
  kParamStochastic = 3 // bf16 parameter read, written stochastically
};

template <class Rule>
struct CompactTable {
  void* param[kStepSegs];
  const void* grad[kStepSegs];
  float* master[kStepSegs];
  void* exp_avg[kStepSegs];     // fp32 or bf16 (state_bf16)
  void* exp_avg_sq[kStepSegs];  //
  int64_t numel[kStepSegs];
  int64_t elem_offset[kStepSegs];  // the piece's first element inside its parameter, a multiple of 4
  typename Rule::Scalars sc[kStepSegs];
  int32_t first_chunk[kStepSegs + 1];
  uint32_t step[kStepSegs];     // counter word 2
  uint32_t ordinal[kStepSegs];  // counter word 3
  uint8_t param_mode[kStepSegs];
  uint8_t grad_bf16[kStepSegs];
  uint8_t state_bf16[kStepSegs];
  uint64_t seed;
  int32_t n;
};
static_assert(sizeof(CompactTable<AdamwRule>) + sizeof(void*) <= 4096, "the table and the record pointer must fit 4 KB of kernel arguments");
static_assert(sizeof(CompactTable<LionRule>) + sizeof(void*) <= 4096, "the table and the record pointer must fit 4 KB of kernel arguments");

__device__ __forceinline__ void apply(const PrlAdamwScalars& s, float coef, float g, float& p, float& m, float& v) { prl_adamw_update(s, coef, g, p, m, v); }
__device__ __forceinline__ void apply(const PrlLionScalars& s, float coef, float g, float& p, float& m, float& v) { prl_lion_update(s, coef, g, p, m); }

// 8 fp32 values -> 8 bf16 with the given 16-bit random values, one 16-byte store
template <bool STREAM>
__device__ __forceinline__ void store8_bf16_sr(void* base, int64_t i, const float (&v)[kGroup], const uint32_t (&r)[kGroup]) {
  u32x4 t;
#pragma unroll
  for (int k = 0; k < 4; ++k) t[k] = (uint32_t)prl_f32_to_bf16_sr(v[2 * k], r[2 * k]) | ((uint32_t)prl_f32_to_bf16_sr(v[2 * k + 1], r[2 * k + 1]) << 16);
  u32x4* p = reinterpret_cast<u32x4*>(static_cast<uint16_t*>(base) + i);
  if constexpr (STREAM) __builtin_nontemporal_store(t, p);  // optimizer state: touched once per step
  else *p = t;                                              // the parameter is read again by the next forward
}

struct Counter {
  int64_t first;  // index inside the parameter of the chunk's first element (a multiple of 4)
  uint32_t step, ordinal;
  uint64_t seed;
};

// One chunk.  PM: ParamMode; GB: bf16 gradient; SB: bf16 state.
template <class Rule, int PM, bool GB, bool SB>
__device__ __forceinline__ void chunk_step(const typename Rule::Scalars sc, float coef, void* param, const void* grad, float* master, void* m_ptr,
                                           void* v_ptr, int64_t len, const Counter ctr) {
  constexpr bool V = Rule::kSecondMoment;
  constexpr bool MW = PM == kParamMaster;
  constexpr bool PB = PM != kParamF32;
  constexpr bool PSR = PM == kParamStochastic;
  constexpr bool RANDOM = SB || PSR;          // something is stored stochastically
  constexpr bool WB = MW ? false : PB;        // dtype of the array the weights are READ from
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
      load8<SB>(m_ptr, i, m);
      if constexpr (V) load8<SB>(v_ptr, i, v);
      uint32_t x[kGroup];
      if constexpr (RANDOM) {  // independent of the loads: issued under their latency
        const uint64_t group = uint64_t(ctr.first + i) >> 2;
        const PrlPhilox4 a = prl_sr_words(group, ctr.step, ctr.ordinal, ctr.seed);
        const PrlPhilox4 b = prl_sr_words(group + 1, ctr.step, ctr.ordinal, ctr.seed);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          x[k] = a.w[k];
          x[4 + k] = b.w[k];
        }
      }
#pragma unroll
      for (int k = 0; k < kGroup; ++k) apply(sc, coef, g[k], w[k], m[k], v[k]);
      if constexpr (SB) {
        uint32_t r[kGroup];
#pragma unroll
        for (int k = 0; k < kGroup; ++k) r[k] = prl_sr_rm(x[k]);
        store8_bf16_sr<true>(m_ptr, i, m, r);
        if constexpr (V) {
#pragma unroll
          for (int k = 0; k < kGroup; ++k) r[k] = prl_sr_rv(x[k]);
          store8_bf16_sr<true>(v_ptr, i, v, r);
        }
      } else {
        store8_stream(static_cast<float*>(m_ptr), i, m);
        if constexpr (V) store8_stream(static_cast<float*>(v_ptr), i, v);
      }
      if constexpr (MW) store8_stream(master, i, w);
      if constexpr (PSR) {
        uint32_t r[kGroup];
#pragma unroll
        for (int k = 0; k < kGroup; ++k) r[k] = prl_sr_rp(x[k]);
        store8_bf16_sr<false>(param, i, w, r);
      } else {
        store8<PB>(param, i, w);
      }
    }
    done = ngroups * kGroup;
  }
  for (int64_t i = done + threadIdx.x; i < len; i += kBlock) {  // tail, or a whole unaligned view
    float w = load1<WB>(w_src, i), m = load1<SB>(m_ptr, i), v = 0.0f;
    if constexpr (V) v = load1<SB>(v_ptr, i);
    apply(sc, coef, load1<GB>(grad, i), w, m, v);
    uint32_t x = 0;
    if constexpr (RANDOM) {
      const uint64_t e = uint64_t(ctr.first + i);
      x = prl_sr_word(prl_sr_words(e >> 2, ctr.step, ctr.ordinal, ctr.seed), uint32_t(e & 3));
    }
    if constexpr (SB) {
      static_cast<uint16_t*>(m_ptr)[i] = prl_f32_to_bf16_sr(m, prl_sr_rm(x));
      if constexpr (V) static_cast<uint16_t*>(v_ptr)[i] = prl_f32_to_bf16_sr(v, prl_sr_rv(x));
    } else {
      static_cast<float*>(m_ptr)[i] = m;
      if constexpr (V) static_cast<float*>(v_ptr)[i] = v;
    }
    if constexpr (MW) master[i] = w;
    if constexpr (PSR) static_cast<uint16_t*>(param)[i] = prl_f32_to_bf16_sr(w, prl_sr_rp(x));
    else store1<PB>(param, i, w);
  }
}

template <class Rule>
struct ChunkArgs {
  typename Rule::Scalars sc;
  float coef;
  void* param;
  const void* grad;
  float* master;
  void* m;
  void* v;
  int64_t len;
  Counter ctr;
};

template <class Rule, int PM>
__device__ __forceinline__ void by_grad_and_state(const ChunkArgs<Rule>& a, bool gb, bool sb) {
  if (gb) {
    if (sb) chunk_step<Rule, PM, true, true>(a.sc, a.coef, a.param, a.grad, a.master, a.m, a.v, a.len, a.ctr);
    else chunk_step<Rule, PM, true, false>(a.sc, a.coef, a.param, a.grad, a.master, a.m, a.v, a.len, a.ctr);
  } else {
    if (sb) chunk_step<Rule, PM, false, true>(a.sc, a.coef, a.param, a.grad, a.master, a.m, a.v, a.len, a.ctr);
    else chunk_step<Rule, PM, false, false>(a.sc, a.coef, a.param, a.grad, a.master, a.m, a.v, a.len, a.ctr);
  }
}

template <class Rule>
__global__ __launch_bounds__(kBlock) void optim_step_compact_kernel(const CompactTable<Rule> tab, const float* __restrict__ norm_and_coef) {
  const int chunk = blockIdx.x;
  const int s = owner(tab.first_chunk, tab.n, chunk);
  const int64_t begin = int64_t(chunk - tab.first_chunk[s]) * kChunk;
  const int64_t left = tab.numel[s] - begin;
  const int pm = tab.param_mode[s];
  const bool gb = tab.grad_bf16[s], sb = tab.state_bf16[s];
  const int64_t pe = pm == kParamF32 ? 4 : 2, ge = gb ? 2 : 4, se = sb ? 2 : 4;
  ChunkArgs<Rule> a;
  a.sc = tab.sc[s];
  a.coef = norm_and_coef ? norm_and_coef[1] : 1.0f;
  a.param = static_cast<char*>(tab.param[s]) + begin * pe;
  a.grad = static_cast<const char*>(tab.grad[s]) + begin * ge;
  a.master = pm == kParamMaster ? tab.master[s] + begin : nullptr;
  a.m = static_cast<char*>(tab.exp_avg[s]) + begin * se;
  a.v = Rule::kSecondMoment ? static_cast<char*>(tab.exp_avg_sq[s]) + begin * se : nullptr;
  a.len = left < kChunk ? left : kChunk;
  a.ctr.first = tab.elem_offset[s] + begin;
  a.ctr.step = tab.step[s];
  a.ctr.ordinal = tab.ordinal[s];
  a.ctr.seed = tab.seed;
  // wave-uniform dispatch on the segment's dtypes and rounding
  switch (pm) {
    case kParamF32: by_grad_and_state<Rule, kParamF32>(a, gb, sb); break;
    case kParamMaster: by_grad_and_state<Rule, kParamMaster>(a, gb, sb); break;
    case kParamNearest: by_grad_and_state<Rule, kParamNearest>(a, gb, sb); break;
    default: by_grad_and_state<Rule, kParamStochastic>(a, gb, sb); break;
  }
}

int64_t chunks_of(int64_t numel) { return (numel + kChunk - 1) / kChunk; }
bool live(const prl_optim_compact_segment& s) { return s.grad != nullptr && s.numel > 0; }

int validate(const prl_optim_compact_segment* segs, int64_t n, bool need_second) {
  PRL_CHECK_ARG(n >= 0, "negative segment count");
  PRL_CHECK_ARG(n == 0 || segs != nullptr, "null segment table with %lld segments", (long long)n);
  for (int64_t i = 0; i < n; ++i) {
    const prl_optim_compact_segment& s = segs[i];
    PRL_CHECK_ARG(s.numel >= 0, "segment %lld: negative numel %lld", (long long)i, (long long)s.numel);
    PRL_CHECK_ARG(chunks_of(s.numel) < (int64_t(1) << 30), "segment %lld: %lld elements are too many for one launch", (long long)i, (long long)s.numel);
    PRL_CHECK_ARG(s.grad_dtype == PRL_DTYPE_F32 || s.grad_dtype == PRL_DTYPE_BF16, "segment %lld: unknown grad_dtype %d", (long long)i, s.grad_dtype);
    PRL_CHECK_ARG(s.param_dtype == PRL_DTYPE_F32 || s.param_dtype == PRL_DTYPE_BF16, "segment %lld: unknown param_dtype %d", (long long)i, s.param_dtype);
    PRL_CHECK_ARG(s.state_dtype == PRL_DTYPE_F32 || s.state_dtype == PRL_DTYPE_BF16, "segment %lld: unknown state_dtype %d", (long long)i, s.state_dtype);
    PRL_CHECK_ARG(s.param_rounding == PRL_ROUND_NEAREST || s.param_rounding == PRL_ROUND_STOCHASTIC, "segment %lld: unknown param_rounding %d", (long long)i,
                  s.param_rounding);
    PRL_CHECK_ARG(s.elem_offset >= 0, "segment %lld: negative elem_offset %lld", (long long)i, (long long)s.elem_offset);
    PRL_CHECK_ARG(s.elem_offset % 4 == 0, "segment %lld: elem_offset %lld is not a multiple of 4 (a group of 4 elements shares one generator call)",
                  (long long)i, (long long)s.elem_offset);
    PRL_CHECK_ARG(s.ordinal >= 0 && s.ordinal <= int64_t(0xffffffffu), "segment %lld: ordinal %lld outside [0, 2^32)", (long long)i, (long long)s.ordinal);
    if (!live(s)) continue;
    PRL_CHECK_ARG(s.param != nullptr && s.exp_avg != nullptr, "segment %lld: null param or exp_avg", (long long)i);
    PRL_CHECK_ARG(!need_second || s.exp_avg_sq != nullptr, "segment %lld: null exp_avg_sq", (long long)i);
    PRL_CHECK_ARG(s.master == nullptr || s.param_dtype == PRL_DTYPE_BF16, "segment %lld: master weights go with a bf16 parameter", (long long)i);
    PRL_CHECK_ARG(s.param_rounding == PRL_ROUND_NEAREST || s.master == nullptr,
                  "segment %lld: stochastic param_rounding with master weights (the master is the truth; the parameter is its nearest image)", (long long)i);
    PRL_CHECK_ARG(s.step >= 1, "segment %lld: step %lld (the number of this update) must be >= 1", (long long)i, (long long)s.step);
  }
  return PRL_OK;
}

void fill_scalars(PrlAdamwScalars& o, const prl_optim_compact_segment& s, double beta1, double beta2, double eps) {
  o = prl_adamw_scalars(s.lr, s.weight_decay, beta1, beta2, eps, s.step);
}
void fill_scalars(PrlLionScalars& o, const prl_optim_compact_segment& s, double beta1, double beta2, double) { o = prl_lion_scalars(s.lr, s.weight_decay, beta1, beta2); }

template <class Rule>
int step_launches(const prl_optim_compact_segment* segs, int64_t n, double beta1, double beta2, double eps, uint64_t seed, const float* norm_and_coef,
                  hipStream_t stream) {
  int64_t i = 0;
  while (i < n) {
    CompactTable<Rule> tab;
    tab.n = 0;
    tab.seed = seed;
    tab.first_chunk[0] = 0;
    int64_t chunks = 0;
    for (; i < n && tab.n < kStepSegs; ++i) {
      const prl_optim_compact_segment& s = segs[i];
      if (!live(s)) continue;
      const int64_t c = chunks_of(s.numel);
      if (chunks + c > (int64_t(1) << 30)) break;  // keep the grid and the prefix sums in int32
      const int k = tab.n;
      tab.param[k] = s.param;
      tab.grad[k] = s.grad;
      tab.master[k] = static_cast<float*>(s.master);
      tab.exp_avg[k] = s.exp_avg;
      tab.exp_avg_sq[k] = s.exp_avg_sq;
      tab.numel[k] = s.numel;
      tab.elem_offset[k] = s.elem_offset;
      tab.step[k] = uint32_t(s.step);
      tab.ordinal[k] = uint32_t(s.ordinal);
      tab.param_mode[k] = s.param_dtype == PRL_DTYPE_F32 ? kParamF32
                          : s.master != nullptr          ? kParamMaster
                          : s.param_rounding == PRL_ROUND_STOCHASTIC ? kParamStochastic
                                                                     : kParamNearest;
      tab.grad_bf16[k] = s.grad_dtype == PRL_DTYPE_BF16;
      tab.state_bf16[k] = s.state_dtype == PRL_DTYPE_BF16;
      fill_scalars(tab.sc[k], s, beta1, beta2, eps);
      chunks += c;
      tab.first_chunk[++tab.n] = int32_t(chunks);
    }
    if (tab.n == 0) break;  // only skipped segments were left (validate() bounds every single segment)
    hipLaunchKernelGGL(optim_step_compact_kernel<Rule>, dim3(unsigned(chunks)), dim3(kBlock), 0, stream, tab, norm_and_coef);
    PRL_LAUNCH_CHECK("optim_step_compact_kernel");
  }
  return PRL_OK;
}

}  // namespace

extern "C" int prl_optim_adamw_step_compact(const prl_optim_compact_segment* segments, int64_t n_segments, double beta1, double beta2, double eps,
                                            uint64_t seed, const float* norm_and_coef, prl_stream_t stream) {
  if (int rc = validate(segments, n_segments, true)) return rc;
  PRL_CHECK_ARG(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "betas (%g, %g) outside [0, 1)", beta1, beta2);
  PRL_CHECK_ARG(eps >= 0.0, "negative eps %g", eps);
  return step_launches<AdamwRule>(segments, n_segments, beta1, beta2, eps, seed, norm_and_coef, static_cast<hipStream_t>(stream));
}

extern "C" int prl_optim_lion_step_compact(const prl_optim_compact_segment* segments, int64_t n_segments, double beta1, double beta2, uint64_t seed,
                                           const float* norm_and_coef, prl_stream_t stream) {
  if (int rc = validate(segments, n_segments, false)) return rc;
  PRL_CHECK_ARG(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "betas (%g, %g) outside [0, 1)", beta1, beta2);
  return step_launches<LionRule>(segments, n_segments, beta1, beta2, 0.0, seed, norm_and_coef, static_cast<hipStream_t>(stream));
}
