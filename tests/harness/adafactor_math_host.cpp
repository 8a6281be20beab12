/* Host build of the DEVICE Adafactor math (pipelinerl_amd/csrc/prl_adafactor_math.h): one step of one parameter with the
 * pieces the HIP kernels execute, the sums taken in fp64 as the kernels take them (their order differs: tiles and bands), so
 * that the rule can be checked against transformers' Adafactor on a machine without a GPU.  Test-only: nothing in the product
 * links or calls this. */
#include "../../pipelinerl_amd/csrc/prl_adafactor_math.h"

#include <vector>

/* factored: p, g are [B, R, C], row [B, R], col [B, C], v unused.  Otherwise B = R = 1 and v has C elements. */
extern "C" void prl_host_adafactor(long B, long R, long C, int factored, double lr, double wd, double eps1, double clip_threshold,
                                   double decay_rate, long step, float coef, const float* g, float* p, float* row, float* col, float* v) {
  const PrlAdafactorScalars s = prl_adafactor_scalars(lr, wd, decay_rate, step);
  const long n = B * R * C;
  std::vector<float> u(n);
  if (factored) {
    for (long b = 0; b < B; ++b) {
      const float* gb = g + b * R * C;
      for (long r = 0; r < R; ++r) {
        double t = 0.0;
        for (long c = 0; c < C; ++c) t += prl_adafactor_sq(prl_adafactor_grad(gb[r * C + c], coef), eps1);
        row[b * R + r] = prl_adafactor_average(s, row[b * R + r], t / (double)C);
      }
      for (long c = 0; c < C; ++c) {
        double t = 0.0;
        for (long r = 0; r < R; ++r) t += prl_adafactor_sq(prl_adafactor_grad(gb[r * C + c], coef), eps1);
        col[b * C + c] = prl_adafactor_average(s, col[b * C + c], t / (double)R);
      }
      double rs = 0.0;
      for (long r = 0; r < R; ++r) rs += (double)row[b * R + r];
      const double row_mean = rs / (double)R;
      for (long r = 0; r < R; ++r) {
        const float rf = prl_adafactor_row_factor(row[b * R + r], row_mean);
        for (long c = 0; c < C; ++c)
          u[b * R * C + r * C + c] = prl_adafactor_update(rf, prl_adafactor_rsqrt(col[b * C + c]), prl_adafactor_grad(gb[r * C + c], coef));
      }
    }
  } else {
    for (long i = 0; i < n; ++i) {
      const float gi = prl_adafactor_grad(g[i], coef);
      v[i] = prl_adafactor_average(s, v[i], prl_adafactor_sq(gi, eps1));
      u[i] = prl_adafactor_update(prl_adafactor_rsqrt(v[i]), 1.0f, gi);
    }
  }
  double ss = 0.0;
  for (long i = 0; i < n; ++i) ss += (double)u[i] * (double)u[i];
  const float denom = prl_adafactor_denom(ss, n, clip_threshold);
  for (long i = 0; i < n; ++i) p[i] = prl_adafactor_apply(s, u[i], denom, p[i]);
}
