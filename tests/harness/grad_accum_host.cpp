/* Host build of the DEVICE gradient-accumulation rule (pipelinerl_amd/csrc/prl_optim_math.h): what one lane of
 * grad_accumulate_kernel does to one element, so that it can be compared with torch bit for bit on a machine without a
 * GPU.  Test-only: nothing in the product links or calls this. */
#include "../../pipelinerl_amd/csrc/prl_optim_math.h"

extern "C" void prl_host_grad_accum_bf16(long n, const uint16_t* g, float* acc, int overwrite) {
  for (long i = 0; i < n; ++i) acc[i] = overwrite ? prl_grad_accum_first(prl_bf16_to_f32(g[i])) : prl_grad_accum_add(acc[i], prl_bf16_to_f32(g[i]));
}

extern "C" void prl_host_grad_accum_f32(long n, const float* g, float* acc, int overwrite) {
  for (long i = 0; i < n; ++i) acc[i] = overwrite ? prl_grad_accum_first(g[i]) : prl_grad_accum_add(acc[i], g[i]);
}
