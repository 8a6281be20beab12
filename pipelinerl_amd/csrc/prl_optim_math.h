// Per-element AdamW / Lion update shared by the multi-tensor step kernels (prl_optim.hip) and the
// host-compiled unit-test harness (tests/harness/optim_math_host.cpp).
//
// Follows, operation by operation in fp32 (build with -ffp-contract=off; the FMAs torch's CPU kernels
// issue themselves - lerp, addcmul, add with alpha - are requested explicitly):
//   * torch.optim.AdamW, single-tensor path (foreach=False, amsgrad=False, decoupled decay):
//       param.mul_(1 - lr * wd)                               one multiply, skipped when wd == 0
//       exp_avg.lerp_(grad, 1 - beta1)                        fma(w, grad - m, m)  (w < 0.5)
//       exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1-beta2)  fma((1-b2)*g, g, v*b2)
//       denom = (exp_avg_sq.sqrt() / bc2_sqrt).add_(eps)      IEEE sqrt and divide (torch's CPU sqrt is a vector-library
//                                                             routine that is 1 ulp off on ~0.7 % of inputs; exp_avg and
//                                                             exp_avg_sq are bit-equal to torch, param is wherever that sqrt is)
//       param.addcdiv_(exp_avg, denom, value=-step_size)      p + ((-step_size)*m)/denom
//   * the reference's Lion.step (pipelinerl/finetune/optim.py:88-110):
//       p.mul_(1 - lr * wd)                                   always, also for wd == 0
//       update = exp_avg * beta1 + grad * (1 - beta1)
//       p.add_(sign(update), alpha=-lr)
//       exp_avg.mul_(beta2).add_(grad, alpha=1 - beta2)       fma(grad, 1-b2, m*b2)
// Python forms every scalar in double and the kernels of torch round it to fp32 once; the
// `prl_*_scalars` helpers below do the same on the host, so the device sees the same fp32 constants.
//
// The gradient is multiplied by the clip coefficient on the way in (what clip_grad_norm_'s
// `g.mul_(clip_coef)` leaves behind, without writing it back).
//
// Gradient accumulation (grad_accumulate_kernel): the micro-batch gradient is widened to fp32 (exact for bf16)
// and added to the fp32 accumulator with ONE IEEE add, no scaling: `acc + g.float()` of torch, bit for bit.
// The first fold of a step stores the widened gradient and never reads the accumulator.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define PRL_OPT_HD __host__ __device__ __forceinline__
#else
#define PRL_OPT_HD static inline
#endif

// fp32 constants of one AdamW step of one parameter
struct PrlAdamwScalars {
  float decay;      // 1 - lr * wd          (applied only when has_decay)
  float w1;         // 1 - beta1            (lerp weight)
  float beta2;      //
  float omb2;       // 1 - beta2
  float bc2_sqrt;   // (1 - beta2^step)^0.5
  float eps;        //
  float neg_step;   // -(lr / (1 - beta1^step))
  int has_decay;    // wd != 0
  int lerp_small;   // |w1| < 0.5: torch's lerp picks m + w (g - m), else g - (g - m)(1 - w)
};

struct PrlLionScalars {
  float decay;   // 1 - lr * wd
  float beta1;   //
  float omb1;    // 1 - beta1
  float beta2;   //
  float omb2;    // 1 - beta2
  float neg_lr;  // -lr
};

// `step` is the number of THIS update (torch increments state["step"] first): 1 for the first one.
static inline PrlAdamwScalars prl_adamw_scalars(double lr, double wd, double beta1, double beta2, double eps, int64_t step) {
  PrlAdamwScalars s;
  const double bc1 = 1.0 - pow(beta1, (double)step);
  const double bc2 = 1.0 - pow(beta2, (double)step);
  s.decay = (float)(1.0 - lr * wd);
  s.w1 = (float)(1.0 - beta1);
  s.beta2 = (float)beta2;
  s.omb2 = (float)(1.0 - beta2);
  s.bc2_sqrt = (float)pow(bc2, 0.5);
  s.eps = (float)eps;
  s.neg_step = (float)(-(lr / bc1));
  s.has_decay = wd != 0.0;
  s.lerp_small = fabs(1.0 - beta1) < 0.5;
  return s;
}

static inline PrlLionScalars prl_lion_scalars(double lr, double wd, double beta1, double beta2) {
  PrlLionScalars s;
  s.decay = (float)(1.0 - lr * wd);
  s.beta1 = (float)beta1;
  s.omb1 = (float)(1.0 - beta1);
  s.beta2 = (float)beta2;
  s.omb2 = (float)(1.0 - beta2);
  s.neg_lr = (float)(-lr);
  return s;
}

PRL_OPT_HD float prl_bf16_to_f32(uint16_t h) {
  const uint32_t u = (uint32_t)h << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}

// round to nearest even, NaN -> the quiet NaN c10::BFloat16 writes (0x7FC0)
PRL_OPT_HD uint16_t prl_f32_to_bf16_rne(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0;
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

// clip_grad_norm_'s coefficient from the fp32 total norm: clamp(max_norm / (norm + 1e-6), max=1); a NaN stays a NaN.
// max_norm <= 0 means "no clipping".
PRL_OPT_HD float prl_clip_coef(float total_norm, float max_norm) {
  if (!(max_norm > 0.0f)) return 1.0f;
  const float c = max_norm / (total_norm + 1e-6f);
  return c > 1.0f ? 1.0f : c;
}

// p, m, v are updated in place; g is the raw gradient, coef the clip coefficient.
PRL_OPT_HD void prl_adamw_update(const PrlAdamwScalars& s, float coef, float g, float& p, float& m, float& v) {
  g = g * coef;
  if (s.has_decay) p = p * s.decay;
  const float diff = g - m;
  m = s.lerp_small ? __builtin_fmaf(s.w1, diff, m) : __builtin_fmaf(s.w1 - 1.0f, diff, g);
  v = v * s.beta2;
  v = __builtin_fmaf(s.omb2 * g, g, v);
  const float denom = sqrtf(v) / s.bc2_sqrt + s.eps;
  p = p + (s.neg_step * m) / denom;
}

PRL_OPT_HD void prl_lion_update(const PrlLionScalars& s, float coef, float g, float& p, float& m) {
  g = g * coef;
  p = p * s.decay;
  const float update = m * s.beta1 + g * s.omb1;
  const float sgn = (float)((update > 0.0f) - (update < 0.0f));  // torch.sign: 0 -> 0; a NaN compares false both ways ...
  p = (update != update) ? update : __builtin_fmaf(sgn, s.neg_lr, p);  // ... and torch.sign(NaN) is NaN
  m = __builtin_fmaf(g, s.omb2, m * s.beta2);
}

// One micro-batch gradient folded into the fp32 accumulator: the first fold of a step / every later one.
PRL_OPT_HD float prl_grad_accum_first(float g) { return g; }
PRL_OPT_HD float prl_grad_accum_add(float acc, float g) { return acc + g; }
