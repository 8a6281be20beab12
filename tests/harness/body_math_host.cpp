/* Host build of the DEVICE math of the fused body kernels (pipelinerl_amd/csrc/prl_body_math.h): RMSNorm and SwiGLU with the
 * per-element pieces the HIP kernels execute, every sum taken in the kernels' own order (a lane's groups of V elements one after
 * the other, the 64 lanes by butterfly; dw: the four waves' rows, then the waves, then the bands), so that the arithmetic can be
 * checked against fp64 on a machine without a GPU.  Values are fp32 here; rounding a result to bf16 is the caller's business.
 * Test-only: nothing in the product links or calls this. */
#include "../../pipelinerl_amd/csrc/prl_body_math.h"

#include <vector>

namespace {

const int kLanes = PRL_BODY_WAVE;
const int kWaves = PRL_BODY_ROWS_PER_BLOCK;

/* prl::wave_sum: v += shfl_xor(v, o) for o = 32 .. 1 */
float butterfly(float (&v)[PRL_BODY_WAVE]) {
  for (int o = kLanes / 2; o > 0; o >>= 1) {
    float t[PRL_BODY_WAVE];
    for (int l = 0; l < kLanes; ++l) t[l] = v[l] + v[l ^ o];
    for (int l = 0; l < kLanes; ++l) v[l] = t[l];
  }
  return v[0];
}

/* the row sum of term(c) as a wave forms it with V elements per lane and iteration */
template <class F>
float row_sum(long cols, int V, F term) {
  float lane[PRL_BODY_WAVE];
  for (int l = 0; l < kLanes; ++l) {
    float acc = 0.0f;
    for (long c = (long)l * V; c < cols; c += (long)kLanes * V) {
      float t[8];
      for (int k = 0; k < V; ++k) t[k] = c + k < cols ? term(c + k) : 0.0f;
      acc = acc + prl_body_sum_group(t, V);
    }
    lane[l] = acc;
  }
  return butterfly(lane);
}

}  // namespace

extern "C" int prl_host_body_geometry(int* out) {
  const int g[] = {PRL_BODY_BLOCK, PRL_BODY_WAVE, PRL_BODY_ROWS_PER_BLOCK, PRL_BODY_VEC_BF16, PRL_BODY_VEC_F32, PRL_BODY_BAND_ROWS, PRL_BODY_SWIGLU_VEC};
  for (int i = 0; i < 7; ++i) out[i] = g[i];
  return 7;
}

extern "C" void prl_host_rmsnorm_fwd(long rows, long cols, int V, const float* x, const float* w, float eps, float* out, float* rstd) {
  for (long r = 0; r < rows; ++r) {
    const float* xr = x + r * cols;
    const float rs = prl_rms_rstd(row_sum(cols, V, [&](long c) { return prl_rms_sq(xr[c]); }), cols, eps);
    rstd[r] = rs;
    for (long c = 0; c < cols; ++c) out[r * cols + c] = prl_rms_out(w[c], xr[c], rs);
  }
}

extern "C" void prl_host_rmsnorm_bwd(long rows, long cols, int V, const float* x, const float* w, const float* rstd, const float* g, float* dx, float* dw) {
  for (long r = 0; r < rows; ++r) {
    const float* xr = x + r * cols;
    const float* gr = g + r * cols;
    const float rs = rstd[r];
    const float cm = prl_rms_row_mean(row_sum(cols, V, [&](long c) { return prl_rms_gwx(gr[c], w[c], xr[c], rs); }), cols);
    for (long c = 0; c < cols; ++c) dx[r * cols + c] = prl_rms_dx(gr[c], w[c], xr[c], rs, cm);
  }
  const long bands = (rows + PRL_BODY_BAND_ROWS - 1) / PRL_BODY_BAND_ROWS;
  for (long c = 0; c < cols; ++c) {
    double total = 0.0;
    for (long b = 0; b < bands; ++b) {
      const long r0 = b * PRL_BODY_BAND_ROWS, r1 = r0 + PRL_BODY_BAND_ROWS < rows ? r0 + PRL_BODY_BAND_ROWS : rows;
      float wave[8] = {0};
      for (int wv = 0; wv < kWaves; ++wv)
        for (long r = r0 + wv; r < r1; r += kWaves) wave[wv] = wave[wv] + prl_rms_dw_term(g[r * cols + c], x[r * cols + c], rstd[r]);
      total += (double)(((wave[0] + wave[1]) + wave[2]) + wave[3]);
    }
    dw[c] = (float)total;
  }
}

extern "C" void prl_host_swiglu_fwd(long n, const float* gate, const float* up, float* out) {
  for (long i = 0; i < n; ++i) out[i] = prl_swiglu_fwd(gate[i], up[i]);
}

extern "C" void prl_host_swiglu_bwd(long n, const float* gate, const float* up, const float* g, float* d_gate, float* d_up) {
  for (long i = 0; i < n; ++i) prl_swiglu_bwd(gate[i], up[i], g[i], d_gate[i], d_up[i]);
}
