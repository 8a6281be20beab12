/* Host build of the rounding rule of the compact optimizer step (pipelinerl_amd/csrc/prl_optim_sr.h): the generator, the
 * stochastic rounding and the per-element compact AdamW / Lion update as the scalar path of csrc/prl_optim_compact.hip composes
 * them (widen, prl_adamw_update / prl_lion_update, round the stores), so that they can be checked bit for bit on a machine
 * without a GPU.  Test-only: nothing in the product links or calls this. */
#include "../../pipelinerl_amd/csrc/prl_optim_sr.h"

extern "C" void prl_host_philox4x32_10(const uint32_t* counter, const uint32_t* key, uint32_t* out) {
  const PrlPhilox4 o = prl_philox4x32_10(counter[0], counter[1], counter[2], counter[3], key[0], key[1]);
  for (int j = 0; j < 4; ++j) out[j] = o.w[j];
}

/* x[i] = the output word of element elem_offset + i */
extern "C" void prl_host_sr_words(long n, long elem_offset, long step, long ordinal, uint64_t seed, uint32_t* x) {
  for (long i = 0; i < n; ++i) {
    const uint64_t e = (uint64_t)(elem_offset + i);
    x[i] = prl_sr_word(prl_sr_words(e >> 2, (uint32_t)step, (uint32_t)ordinal, seed), (uint32_t)(e & 3));
  }
}

extern "C" uint16_t prl_host_sr(float f, uint32_t r) { return prl_f32_to_bf16_sr(f, r); }

/* out[r] = sr(f, r) for every r in 0 .. 65535 */
extern "C" void prl_host_sr_all(float f, uint16_t* out) {
  for (uint32_t r = 0; r < 65536u; ++r) out[r] = prl_f32_to_bf16_sr(f, r);
}

namespace {

float load(const void* a, long i, int bf16) { return bf16 ? prl_bf16_to_f32(static_cast<const uint16_t*>(a)[i]) : static_cast<const float*>(a)[i]; }

/* param_mode: 0 fp32 parameter | 1 bf16 parameter + fp32 master | 2 bf16 parameter to nearest | 3 bf16 parameter stochastic */
template <class Update>
void compact_step(long n, float coef, const float* g, void* p, float* master, void* m, void* v, int param_mode, int state_bf16, long elem_offset,
                  long step, long ordinal, uint64_t seed, Update update) {
  for (long i = 0; i < n; ++i) {
    float w = param_mode == 1 ? master[i] : load(p, i, param_mode != 0);
    float mi = load(m, i, state_bf16), vi = v ? load(v, i, state_bf16) : 0.0f;
    update(coef, g[i], w, mi, vi);
    const uint64_t e = (uint64_t)(elem_offset + i);
    const uint32_t x = prl_sr_word(prl_sr_words(e >> 2, (uint32_t)step, (uint32_t)ordinal, seed), (uint32_t)(e & 3));
    if (state_bf16) {
      static_cast<uint16_t*>(m)[i] = prl_f32_to_bf16_sr(mi, prl_sr_rm(x));
      if (v) static_cast<uint16_t*>(v)[i] = prl_f32_to_bf16_sr(vi, prl_sr_rv(x));
    } else {
      static_cast<float*>(m)[i] = mi;
      if (v) static_cast<float*>(v)[i] = vi;
    }
    if (param_mode == 1) master[i] = w;
    if (param_mode == 0) static_cast<float*>(p)[i] = w;
    else static_cast<uint16_t*>(p)[i] = param_mode == 3 ? prl_f32_to_bf16_sr(w, prl_sr_rp(x)) : prl_f32_to_bf16_rne(w);
  }
}

}  // namespace

extern "C" void prl_host_compact_adamw(long n, double lr, double wd, double beta1, double beta2, double eps, long step, float coef, const float* g,
                                       void* p, float* master, void* m, void* v, int param_mode, int state_bf16, long elem_offset, long ordinal,
                                       uint64_t seed) {
  const PrlAdamwScalars s = prl_adamw_scalars(lr, wd, beta1, beta2, eps, step);
  compact_step(n, coef, g, p, master, m, v, param_mode, state_bf16, elem_offset, step, ordinal, seed,
               [&](float c, float gi, float& w, float& mi, float& vi) { prl_adamw_update(s, c, gi, w, mi, vi); });
}

extern "C" void prl_host_compact_lion(long n, double lr, double wd, double beta1, double beta2, long step, float coef, const float* g, void* p,
                                      float* master, void* m, int param_mode, int state_bf16, long elem_offset, long ordinal, uint64_t seed) {
  const PrlLionScalars s = prl_lion_scalars(lr, wd, beta1, beta2);
  compact_step(n, coef, g, p, master, m, nullptr, param_mode, state_bf16, elem_offset, step, ordinal, seed,
               [&](float c, float gi, float& w, float& mi, float&) { prl_lion_update(s, c, gi, w, mi); });
}
