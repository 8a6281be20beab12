// Per-element pieces of the fused RMSNorm and SwiGLU kernels (prl_body.hip), shared with the host-compiled unit-test harness
// (tests/harness/body_math_host.cpp), and the geometry the tests place their shapes by.
//
// RMSNorm (Qwen2RMSNorm / LlamaRMSNorm: weight * (x * rsqrt(mean(x^2) + eps))), everything in fp32 from the stored values:
//   forward   ss = sum over the row of x^2 (fixed order: prl_body_sum_group per lane group, the groups of a lane one after the
//             other, the 64 lanes by butterfly);  rstd = 1 / sqrt(ss / H + eps);  out = w * (x * rstd), rounded ONCE
//   backward  xh = x * rstd;  c = (sum over the row of (g w) xh) / H;  dx = rstd * (g w - xh c);  dw = sum over rows of g xh
// SwiGLU (act_fn = silu):  e = exp(-z);  silu = z / (1 + e);  out = silu * up
//   backward  sigma = 1 / (1 + e);  d_up = g silu;  d_gate = (g up) (1 + z (1 - sigma)) / (1 + e), with 1 - sigma taken as
//             e / (1 + e) for z >= 0 (no cancellation near sigma = 1) and as the subtraction for z < 0 (e may be inf there)
// One exp per element and no other transcendental call.  Build with -ffp-contract=off.
#pragma once

#include "prl_optim_math.h"

// ---- geometry (mirrored in pipelinerl_amd/_lib.py; tests read it from there) ---------------------------------------------
#define PRL_BODY_BLOCK 256          // threads per workgroup, every kernel of prl_body.hip
#define PRL_BODY_WAVE 64            // lanes that share one row of an RMSNorm
#define PRL_BODY_ROWS_PER_BLOCK 4   // RMSNorm forward / dx: one wave per row
#define PRL_BODY_VEC_BF16 8         // RMSNorm: elements per lane and iteration when x is bf16 (16 bytes)
#define PRL_BODY_VEC_F32 4          //          ... when x is fp32 (16 bytes)
#define PRL_BODY_BAND_ROWS 32       // RMSNorm dw: rows per band (one fp32 partial [H] per band in the workspace)
#define PRL_BODY_SWIGLU_VEC 8       // SwiGLU: elements per thread, both dtypes

// the sum of one lane group in a fixed pairwise order (n = 4 or 8)
PRL_OPT_HD float prl_body_sum_group(const float* t, int n) {
  const float a = (t[0] + t[1]) + (t[2] + t[3]);
  if (n == 4) return a;
  return a + ((t[4] + t[5]) + (t[6] + t[7]));
}

// ---- RMSNorm -----------------------------------------------------------------------------------------------------------
PRL_OPT_HD float prl_rms_sq(float x) { return x * x; }

PRL_OPT_HD float prl_rms_rstd(float sum_sq, int64_t cols, float eps) { return 1.0f / sqrtf(sum_sq / (float)cols + eps); }

PRL_OPT_HD float prl_rms_out(float w, float x, float rstd) { return w * (x * rstd); }

// one term of the row sum under c
PRL_OPT_HD float prl_rms_gwx(float g, float w, float x, float rstd) { return (g * w) * (x * rstd); }

PRL_OPT_HD float prl_rms_row_mean(float sum, int64_t cols) { return sum / (float)cols; }

PRL_OPT_HD float prl_rms_dx(float g, float w, float x, float rstd, float c) { return rstd * (g * w - (x * rstd) * c); }

// one term of dw's sum over rows
PRL_OPT_HD float prl_rms_dw_term(float g, float x, float rstd) { return g * (x * rstd); }

// ---- SwiGLU ------------------------------------------------------------------------------------------------------------
PRL_OPT_HD float prl_swiglu_fwd(float z, float up) {
  const float e = expf(-z);
  return (z / (1.0f + e)) * up;
}

PRL_OPT_HD void prl_swiglu_bwd(float z, float up, float g, float& d_gate, float& d_up) {
  const float e = expf(-z);
  const float d = 1.0f + e;
  const float one_minus = z >= 0.0f ? e / d : 1.0f - 1.0f / d;
  d_up = g * (z / d);
  d_gate = ((g * up) * (1.0f + z * one_minus)) / d;  // (... sigma as the LAST step: for z < -87 sigma itself is below the normal range)
}
