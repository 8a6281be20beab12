/* Host build of the DEVICE optimizer math (pipelinerl_amd/csrc/prl_optim_math.h) so that the exact
 * per-element AdamW / Lion updates the HIP kernels execute can be checked against torch and the
 * reference's Lion on a machine without a GPU.  Test-only: nothing in the product links or calls this. */
#include "../../pipelinerl_amd/csrc/prl_optim_math.h"

extern "C" void prl_host_adamw(long n, double lr, double wd, double beta1, double beta2, double eps, long step, float coef,
                               const float* g, float* p, float* m, float* v) {
  const PrlAdamwScalars s = prl_adamw_scalars(lr, wd, beta1, beta2, eps, step);
  for (long i = 0; i < n; ++i) prl_adamw_update(s, coef, g[i], p[i], m[i], v[i]);
}

extern "C" void prl_host_lion(long n, double lr, double wd, double beta1, double beta2, float coef, const float* g, float* p,
                              float* m) {
  const PrlLionScalars s = prl_lion_scalars(lr, wd, beta1, beta2);
  for (long i = 0; i < n; ++i) prl_lion_update(s, coef, g[i], p[i], m[i]);
}

extern "C" void prl_host_bf16_round(long n, const float* x, uint16_t* out) {
  for (long i = 0; i < n; ++i) out[i] = prl_f32_to_bf16_rne(x[i]);
}

extern "C" float prl_host_clip_coef(float total_norm, float max_norm) { return prl_clip_coef(total_norm, max_norm); }
