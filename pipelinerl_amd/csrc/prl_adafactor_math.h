// Per-element and per-table pieces of the Adafactor step shared by the kernels (prl_adafactor.hip) and the host-compiled
// unit-test harness (tests/harness/adafactor_math_host.cpp).
//
// The rule is transformers.optimization.Adafactor.step with relative_step=False, scale_parameter=False, beta1=None
// (what the reference's get_optimizer constructs, pipelinerl/finetune/optim.py:33-36), operation by operation:
//   grad   = grad * clip_coef                                        (what clip_grad_norm_ leaves behind; not written back)
//   beta2t = 1 - step ** decay_rate                                  double on the host, rounded to fp32 once
//   update = grad**2 + eps1
//   factored (>= 2 dimensions; the leading ones are a batch of matrices):
//     row.mul_(beta2t).add_(update.mean(-1), alpha=1 - beta2t)
//     col.mul_(beta2t).add_(update.mean(-2), alpha=1 - beta2t)
//     update = (row / row.mean(-1)).rsqrt()[r] * col.rsqrt()[c] * grad
//   unfactored (1 dimension):
//     v.mul_(beta2t).add_(update, alpha=1 - beta2t);  update = v.rsqrt() * grad
//   update.div_(max(1, rms(update) / clip_threshold));  update.mul_(lr)
//   p.add_(p, alpha=-wd * lr)   only when wd != 0;      p.add_(-update)
// Every sum over more than one element (the two means of update, the mean of row, the sum of squares under the rms) is taken in
// fp64 in a fixed order by the caller and handed to these pieces as a double: squares of fp32 values are exact in fp64.
// Build with -ffp-contract=off.
#pragma once

#include "prl_optim_math.h"

// fp32 constants of one Adafactor step of one parameter
struct PrlAdafactorScalars {
  float beta2t;   // 1 - step^decay_rate
  float omb2t;    // 1 - beta2t
  float lr;       //
  float decay;    // -wd * lr      (applied only when has_decay)
  int has_decay;  // wd != 0
};

// `step` is the number of THIS update: 1 for the first one (beta2t = 0: the averages start from this step's statistics).
static inline PrlAdafactorScalars prl_adafactor_scalars(double lr, double wd, double decay_rate, int64_t step) {
  PrlAdafactorScalars s;
  const double beta2t = 1.0 - pow((double)step, decay_rate);
  s.beta2t = (float)beta2t;
  s.omb2t = (float)(1.0 - beta2t);
  s.lr = (float)lr;
  s.decay = (float)(-wd * lr);
  s.has_decay = wd != 0.0;
  return s;
}

PRL_OPT_HD float prl_adafactor_grad(float raw, float coef) { return raw * coef; }

// grad**2 + eps1 of one element, as the term of an fp64 sum
PRL_OPT_HD double prl_adafactor_sq(float g, double eps1) {
  const double d = (double)g;
  return d * d + eps1;
}

// the moving average of row / col / v: `mean_sq` is the fp64 mean of update over the other axis (v: the element's own update)
PRL_OPT_HD float prl_adafactor_average(const PrlAdafactorScalars& s, float old, double mean_sq) { return old * s.beta2t + (float)mean_sq * s.omb2t; }

PRL_OPT_HD float prl_adafactor_rsqrt(float x) { return 1.0f / sqrtf(x); }

// the row factor: `row_mean` = mean over the rows of one matrix of the NEW row averages
PRL_OPT_HD float prl_adafactor_row_factor(float row, double row_mean) { return prl_adafactor_rsqrt(row / (float)row_mean); }

PRL_OPT_HD float prl_adafactor_update(float row_factor, float col_factor, float g) { return (row_factor * col_factor) * g; }

// max(1, rms(update) / clip_threshold) from the fp64 sum of squares over the WHOLE parameter
PRL_OPT_HD float prl_adafactor_denom(double sum_sq, int64_t numel, double clip_threshold) {
  const float r = (float)(sqrt(sum_sq / (double)numel) / clip_threshold);
  return r > 1.0f ? r : 1.0f;  // a NaN stays out of the comparison's true branch ...
}

// ... and reaches the parameter through `update` itself.  p is the fp32 weight (the master copy of a bf16 parameter).
PRL_OPT_HD float prl_adafactor_apply(const PrlAdafactorScalars& s, float update, float denom, float p) {
  update = update / denom;
  update = update * s.lr;
  if (s.has_decay) p = p + p * s.decay;
  return p - update;
}
