// The two elementwise / row-reduce op chains of a decoder layer's body as single launches: RMSNorm (Qwen2RMSNorm, LlamaRMSNorm,
// ...: 8 eager launches forward, a dozen backward) and SwiGLU (act_fn(gate) * up).  The arithmetic is prl_body_math.h.
//
// RMSNorm forward / dx: one wave per row, four rows per workgroup.  A lane takes V consecutive elements (16 bytes of x: V = 8 for
// bf16, 4 for fp32) per iteration, the columns lane * V + k * 64 V.  Pass 1 reduces the row (x^2 forward, (g w) xh backward: per
// group in a fixed pairwise order, a lane's groups one after the other, the lanes by butterfly), pass 2 writes the result,
// rounded once.  A row of up to 8 iterations (backward, bf16: 4) is loaded once, all loads in flight together, and waits in
// registers for pass 2; a wider one is read again - the wave touched it a few microseconds ago, it comes from L1 / L2.
// 16-byte moves when H % V == 0 and the arrays are 16-byte aligned; otherwise the SAME elements per lane one at a time: the
// arithmetic order of a row does not depend on the path.
// RMSNorm dw, in the launch of dx (the workgroups after the row workgroups): a workgroup owns a band of kBand rows x 64 V
// columns; wave w takes rows w, w + 4, ... of the band, a lane its V columns; the four waves' sums are added in wave order and
// stored as the band's fp32 partial [H] in the workspace; rmsnorm_dw_fold_kernel adds the bands in band order.  No atomics:
// two runs give the same bits.
// SwiGLU: flat, 8 elements per thread (16 bytes of bf16, 2 x 16 of fp32), the ragged last group element by element.
// Algorithmic bytes per element, bf16: RMSNorm forward 2 + 2, backward 2 + 2 + 2 (+ 2 + 2: dw reads x and g again);
// SwiGLU forward 2 + 2 + 2, backward 2 + 2 + 2 + 2 + 2.
#include "prl_common.h"
#include "prl_body_math.h"

namespace {

using prl::kWave;

constexpr int kBlock = PRL_BODY_BLOCK;
constexpr int kWaves = kBlock / kWave;
constexpr int kBand = PRL_BODY_BAND_ROWS;
constexpr int kSwigluVec = PRL_BODY_SWIGLU_VEC;
static_assert(kWave == PRL_BODY_WAVE && kWaves == PRL_BODY_ROWS_PER_BLOCK, "geometry of prl_body_math.h");
constexpr int64_t kMaxGrid = (int64_t(1) << 24) - 1;  // workgroups per launch: grid x block stays below 2^32 threads

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

__host__ __device__ inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---- V (4 or 8) consecutive elements of an fp32 / bf16 array <-> registers ---------------------------------------------
// VEC: the group is whole and starts 16-byte aligned (bf16, V = 4: 8-byte).  Otherwise `n` (<= V) elements one at a time,
// the rest read as 0 / not written.
template <bool BF16, int V, bool VEC>
__device__ __forceinline__ void ldv(const void* base, int64_t e, int n, float (&o)[V]) {
  if constexpr (!VEC) {
#pragma unroll
    for (int k = 0; k < V; ++k)
      o[k] = k < n ? (BF16 ? prl_bf16_to_f32(static_cast<const uint16_t*>(base)[e + k]) : static_cast<const float*>(base)[e + k]) : 0.0f;
  } else if constexpr (BF16) {
    uint32_t t[V / 2];
    if constexpr (V == 8) {
      const u32x4 q = *reinterpret_cast<const u32x4*>(static_cast<const uint16_t*>(base) + e);
      t[0] = q[0], t[1] = q[1], t[2] = q[2], t[3] = q[3];
    } else {
      const u32x2 q = *reinterpret_cast<const u32x2*>(static_cast<const uint16_t*>(base) + e);
      t[0] = q[0], t[1] = q[1];
    }
#pragma unroll
    for (int k = 0; k < V / 2; ++k) {
      o[2 * k] = __uint_as_float(t[k] << 16);
      o[2 * k + 1] = __uint_as_float(t[k] & 0xffff0000u);
    }
  } else {
    const f32x4* p = reinterpret_cast<const f32x4*>(static_cast<const float*>(base) + e);
#pragma unroll
    for (int q = 0; q < V / 4; ++q) {
      const f32x4 a = p[q];
#pragma unroll
      for (int k = 0; k < 4; ++k) o[4 * q + k] = a[k];
    }
  }
}

template <bool BF16, int V, bool VEC>
__device__ __forceinline__ void stv(void* base, int64_t e, int n, const float (&v)[V]) {
  if constexpr (!VEC) {
#pragma unroll
    for (int k = 0; k < V; ++k) {
      if (k < n) {
        if constexpr (BF16) static_cast<uint16_t*>(base)[e + k] = prl_f32_to_bf16_rne(v[k]);
        else static_cast<float*>(base)[e + k] = v[k];
      }
    }
  } else if constexpr (BF16) {
    uint32_t t[V / 2];
#pragma unroll
    for (int k = 0; k < V / 2; ++k) t[k] = (uint32_t)prl_f32_to_bf16_rne(v[2 * k]) | ((uint32_t)prl_f32_to_bf16_rne(v[2 * k + 1]) << 16);
    if constexpr (V == 8) *reinterpret_cast<u32x4*>(static_cast<uint16_t*>(base) + e) = u32x4{t[0], t[1], t[2], t[3]};
    else *reinterpret_cast<u32x2*>(static_cast<uint16_t*>(base) + e) = u32x2{t[0], t[1]};
  } else {
    f32x4* p = reinterpret_cast<f32x4*>(static_cast<float*>(base) + e);
#pragma unroll
    for (int q = 0; q < V / 4; ++q) p[q] = f32x4{v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
  }
}

// The registers of one whole group as loaded (16 bytes of bf16 / fp32 x; a bf16 group of 4: 8 bytes; an fp32 group of 8: 2 x 16).
template <bool BF16, int V>
struct Raw {
  static constexpr int kWords = BF16 ? V / 2 : V;
  uint32_t u[kWords];
  __device__ __forceinline__ void load(const void* base, int64_t e) {
    if constexpr (kWords == 2) {
      const u32x2 q = *reinterpret_cast<const u32x2*>(static_cast<const uint16_t*>(base) + e);
      u[0] = q[0], u[1] = q[1];
    } else {
      const u32x4* p = BF16 ? reinterpret_cast<const u32x4*>(static_cast<const uint16_t*>(base) + e)
                            : reinterpret_cast<const u32x4*>(static_cast<const float*>(base) + e);
#pragma unroll
      for (int q = 0; q < kWords / 4; ++q) {
        const u32x4 a = p[q];
#pragma unroll
        for (int k = 0; k < 4; ++k) u[4 * q + k] = a[k];
      }
    }
  }
  // The words as they are, opaque to the optimiser: what was unpacked from them before this point is not kept alive
  // across it (the unpacked row is twice the registers of the packed one), the second pass unpacks again.
  __device__ __forceinline__ void pin() {
#pragma unroll
    for (int k = 0; k < kWords; ++k) asm volatile("" : "+v"(u[k]));
  }
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int k = 0; k < kWords; ++k) u[k] = 0u;
  }
  __device__ __forceinline__ void unpack(float (&o)[V]) const {
    if constexpr (BF16) {
#pragma unroll
      for (int k = 0; k < V / 2; ++k) {
        o[2 * k] = __uint_as_float(u[k] << 16);
        o[2 * k + 1] = __uint_as_float(u[k] & 0xffff0000u);
      }
    } else {
#pragma unroll
      for (int k = 0; k < V; ++k) o[k] = __uint_as_float(u[k]);
    }
  }
};

// XB / WB: bf16 x / weight.  The output (and the gradient that comes back for it) is bf16 only when both are: torch promotion.
template <bool XB>
struct Vec { static constexpr int n = XB ? PRL_BODY_VEC_BF16 : PRL_BODY_VEC_F32; };

// ITERS > 0 (16-byte path only): the row fits ITERS iterations of the wave and stays in registers between the two passes - one
// read, all of a lane's loads in flight at once.  ITERS == 0: any width, the second pass reads the row again (L1 / L2).
// Both forms give a lane the same elements in the same order: the same bits.
constexpr int kMaxIters = 8;

// ---- RMSNorm forward --------------------------------------------------------------------------------------------------------
template <bool XB, bool WB, bool VEC, int ITERS>
__global__ __launch_bounds__(kBlock) void rmsnorm_fwd_kernel(const void* __restrict__ x, const void* __restrict__ w, void* __restrict__ out,
                                                             float* __restrict__ rstd_out, int64_t rows, int cols, float eps) {
  constexpr int V = Vec<XB>::n;
  constexpr bool OB = XB && WB;
  static_assert(ITERS == 0 || VEC, "rows are kept in registers on the 16-byte path only");
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t r = int64_t(blockIdx.x) * kWaves + threadIdx.x / kWave;
  if (r >= rows) return;  // (no barrier below)
  const int64_t base = r * cols;
  float acc = 0.0f;
  if constexpr (ITERS > 0) {
    float xv[ITERS][V];
#pragma unroll
    for (int i = 0; i < ITERS; ++i) {
      const int c = (i * kWave + lane) * V;
      if (c < cols) {
        ldv<XB, V, true>(x, base + c, V, xv[i]);
      } else {
#pragma unroll
        for (int k = 0; k < V; ++k) xv[i][k] = 0.0f;
      }
    }
#pragma unroll
    for (int i = 0; i < ITERS; ++i) {
      float t[V];
#pragma unroll
      for (int k = 0; k < V; ++k) t[k] = prl_rms_sq(xv[i][k]);
      acc = acc + prl_body_sum_group(t, V);  // (a group past the row adds +0: the bits of the loop that skips it)
    }
    const float rstd = prl_rms_rstd(prl::wave_sum(acc), cols, eps);
    if (lane == 0) rstd_out[r] = rstd;
#pragma unroll
    for (int i = 0; i < ITERS; ++i) {
      const int c = (i * kWave + lane) * V;
      if (c < cols) {
        float wv[V];
        ldv<WB, V, true>(w, c, V, wv);
#pragma unroll
        for (int k = 0; k < V; ++k) wv[k] = prl_rms_out(wv[k], xv[i][k], rstd);
        stv<OB, V, true>(out, base + c, V, wv);
      }
    }
  } else {
#pragma unroll 4
    for (int c = lane * V; c < cols; c += kWave * V) {
      float xv[V], t[V];
      ldv<XB, V, VEC>(x, base + c, cols - c, xv);
#pragma unroll
      for (int k = 0; k < V; ++k) t[k] = prl_rms_sq(xv[k]);
      acc = acc + prl_body_sum_group(t, V);
    }
    const float rstd = prl_rms_rstd(prl::wave_sum(acc), cols, eps);
    if (lane == 0) rstd_out[r] = rstd;
#pragma unroll 4
    for (int c = lane * V; c < cols; c += kWave * V) {
      float xv[V], wv[V];
      ldv<XB, V, VEC>(x, base + c, cols - c, xv);
      ldv<WB, V, VEC>(w, c, cols - c, wv);
#pragma unroll
      for (int k = 0; k < V; ++k) xv[k] = prl_rms_out(wv[k], xv[k], rstd);
      stv<OB, V, VEC>(out, base + c, cols - c, xv);
    }
  }
}

// ---- RMSNorm backward -------------------------------------------------------------------------------------------------------
// One launch, two kinds of workgroup.  The first `dx_blocks` workgroups: dx, one wave per row like the forward (x and g stay in
// registers as loaded when ITERS > 0).  The `tiles` x `bands` workgroups after them: the band's partial of dw for one tile of
// 64 V columns, partial[band][column] = sum over the band's rows of g xh.
template <bool XB, bool WB, bool VEC, int ITERS>
__device__ __forceinline__ void rmsnorm_dx_rows(const void* __restrict__ x, const void* __restrict__ w, const float* __restrict__ rstd_in,
                                                const void* __restrict__ g, void* __restrict__ dx, int64_t rows, int cols, int block) {
  constexpr int V = Vec<XB>::n;
  constexpr bool OB = XB && WB;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t r = int64_t(block) * kWaves + threadIdx.x / kWave;
  if (r >= rows) return;
  const int64_t base = r * cols;
  const float rstd = rstd_in[r];
  float acc = 0.0f;
  if constexpr (ITERS > 0) {
    Raw<XB, V> xr[ITERS];
    Raw<OB, V> gr[ITERS];
#pragma unroll
    for (int i = 0; i < ITERS; ++i) {
      const int c = (i * kWave + lane) * V;
      if (c < cols) {
        xr[i].load(x, base + c);
        gr[i].load(g, base + c);
      } else {
        xr[i].zero();
        gr[i].zero();
      }
    }
#pragma unroll
    for (int i = 0; i < ITERS; ++i) {
      const int c = (i * kWave + lane) * V;
      float xv[V], gv[V], wv[V];
      xr[i].unpack(xv);
      gr[i].unpack(gv);
      if (c < cols) {
        ldv<WB, V, true>(w, c, V, wv);
      } else {
#pragma unroll
        for (int k = 0; k < V; ++k) wv[k] = 0.0f;
      }
#pragma unroll
      for (int k = 0; k < V; ++k) xv[k] = prl_rms_gwx(gv[k], wv[k], xv[k], rstd);
      acc = acc + prl_body_sum_group(xv, V);
    }
    const float cm = prl_rms_row_mean(prl::wave_sum(acc), cols);
#pragma unroll
    for (int i = 0; i < ITERS; ++i) {
      xr[i].pin();
      gr[i].pin();
    }
#pragma unroll
    for (int i = 0; i < ITERS; ++i) {
      const int c = (i * kWave + lane) * V;
      if (c < cols) {
        float xv[V], gv[V], wv[V];
        xr[i].unpack(xv);
        gr[i].unpack(gv);
        ldv<WB, V, true>(w, c, V, wv);
#pragma unroll
        for (int k = 0; k < V; ++k) xv[k] = prl_rms_dx(gv[k], wv[k], xv[k], rstd, cm);
        stv<XB, V, true>(dx, base + c, V, xv);
      }
    }
  } else {
#pragma unroll 4
    for (int c = lane * V; c < cols; c += kWave * V) {
      float xv[V], wv[V], gv[V];
      ldv<XB, V, VEC>(x, base + c, cols - c, xv);
      ldv<WB, V, VEC>(w, c, cols - c, wv);
      ldv<OB, V, VEC>(g, base + c, cols - c, gv);
#pragma unroll
      for (int k = 0; k < V; ++k) xv[k] = prl_rms_gwx(gv[k], wv[k], xv[k], rstd);
      acc = acc + prl_body_sum_group(xv, V);
    }
    const float cm = prl_rms_row_mean(prl::wave_sum(acc), cols);
#pragma unroll 4
    for (int c = lane * V; c < cols; c += kWave * V) {
      float xv[V], wv[V], gv[V];
      ldv<XB, V, VEC>(x, base + c, cols - c, xv);
      ldv<WB, V, VEC>(w, c, cols - c, wv);
      ldv<OB, V, VEC>(g, base + c, cols - c, gv);
#pragma unroll
      for (int k = 0; k < V; ++k) xv[k] = prl_rms_dx(gv[k], wv[k], xv[k], rstd, cm);
      stv<XB, V, VEC>(dx, base + c, cols - c, xv);
    }
  }
}

template <bool XB, bool OB, bool VEC>
__device__ __forceinline__ void rmsnorm_dw_band(const void* __restrict__ x, const float* __restrict__ rstd_in, const void* __restrict__ g,
                                                float* __restrict__ partial, int64_t rows, int cols, int tile, int band, float (&red)[kWaves][kWave * PRL_BODY_VEC_BF16]) {
  constexpr int V = Vec<XB>::n;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int c = (tile * kWave + lane) * V;  // this lane's first column (may lie past the row)
  const int64_t r0 = int64_t(band) * kBand;
  const int64_t r1 = r0 + kBand < rows ? r0 + kBand : rows;
  float acc[V];
#pragma unroll
  for (int k = 0; k < V; ++k) acc[k] = 0.0f;
  if (c < cols) {
#pragma unroll 4
    for (int64_t r = r0 + wave; r < r1; r += kWaves) {
      const float rstd = rstd_in[r];
      float xv[V], gv[V];
      ldv<XB, V, VEC>(x, r * cols + c, cols - c, xv);
      ldv<OB, V, VEC>(g, r * cols + c, cols - c, gv);
#pragma unroll
      for (int k = 0; k < V; ++k) acc[k] = acc[k] + prl_rms_dw_term(gv[k], xv[k], rstd);
    }
  }
#pragma unroll
  for (int k = 0; k < V; ++k) red[wave][lane * V + k] = acc[k];
  __syncthreads();  // (every thread of a dw workgroup gets here)
  for (int j = threadIdx.x; j < kWave * V; j += kBlock) {
    const int col = tile * kWave * V + j;
    if (col < cols) partial[int64_t(band) * cols + col] = ((red[0][j] + red[1][j]) + red[2][j]) + red[3][j];
  }
}

template <bool XB, bool WB, bool VEC, int ITERS>
__global__ __launch_bounds__(kBlock) void rmsnorm_bwd_kernel(const void* __restrict__ x, const void* __restrict__ w, const float* __restrict__ rstd_in,
                                                             const void* __restrict__ g, void* __restrict__ dx, float* __restrict__ partial, int64_t rows,
                                                             int cols, int dx_blocks, int tiles) {
  __shared__ float red[kWaves][kWave * PRL_BODY_VEC_BF16];
  const int b = int(blockIdx.x);  // (uniform over the workgroup: one kind of work per workgroup)
  if (b < dx_blocks) {
    rmsnorm_dx_rows<XB, WB, VEC, ITERS>(x, w, rstd_in, g, dx, rows, cols, b);
  } else {
    const int t = b - dx_blocks;
    rmsnorm_dw_band<XB, XB && WB, VEC>(x, rstd_in, g, partial, rows, cols, t % tiles, t / tiles, red);
  }
}

__global__ __launch_bounds__(kBlock) void rmsnorm_dw_fold_kernel(const float* __restrict__ partial, float* __restrict__ dw, int bands, int cols) {
  const int col = int(blockIdx.x) * kBlock + threadIdx.x;
  if (col >= cols) return;
  double t = 0.0;
  for (int b = 0; b < bands; ++b) t += double(partial[int64_t(b) * cols + col]);
  dw[col] = float(t);
}

// ---- SwiGLU --------------------------------------------------------------------------------------------------------------
template <bool BF16, bool ALIGNED>
__global__ __launch_bounds__(kBlock) void swiglu_fwd_kernel(const void* __restrict__ gate, const void* __restrict__ up, void* __restrict__ out, int64_t numel) {
  constexpr int V = kSwigluVec;
  const int64_t e = (int64_t(blockIdx.x) * kBlock + threadIdx.x) * V;
  if (e >= numel) return;
  const int n = numel - e < V ? int(numel - e) : V;
  float a[V], b[V];
  if (ALIGNED && n == V) {
    ldv<BF16, V, true>(gate, e, V, a);
    ldv<BF16, V, true>(up, e, V, b);
  } else {
    ldv<BF16, V, false>(gate, e, n, a);
    ldv<BF16, V, false>(up, e, n, b);
  }
#pragma unroll
  for (int k = 0; k < V; ++k) a[k] = prl_swiglu_fwd(a[k], b[k]);
  if (ALIGNED && n == V) stv<BF16, V, true>(out, e, V, a);
  else stv<BF16, V, false>(out, e, n, a);
}

template <bool BF16, bool ALIGNED>
__global__ __launch_bounds__(kBlock) void swiglu_bwd_kernel(const void* __restrict__ gate, const void* __restrict__ up, const void* __restrict__ g,
                                                            void* __restrict__ d_gate, void* __restrict__ d_up, int64_t numel) {
  constexpr int V = kSwigluVec;
  const int64_t e = (int64_t(blockIdx.x) * kBlock + threadIdx.x) * V;
  if (e >= numel) return;
  const int n = numel - e < V ? int(numel - e) : V;
  float a[V], b[V], gv[V];
  if (ALIGNED && n == V) {
    ldv<BF16, V, true>(gate, e, V, a);
    ldv<BF16, V, true>(up, e, V, b);
    ldv<BF16, V, true>(g, e, V, gv);
  } else {
    ldv<BF16, V, false>(gate, e, n, a);
    ldv<BF16, V, false>(up, e, n, b);
    ldv<BF16, V, false>(g, e, n, gv);
  }
#pragma unroll
  for (int k = 0; k < V; ++k) {
    float dg, du;
    prl_swiglu_bwd(a[k], b[k], gv[k], dg, du);
    a[k] = dg, b[k] = du;
  }
  if (ALIGNED && n == V) {
    stv<BF16, V, true>(d_gate, e, V, a);
    stv<BF16, V, true>(d_up, e, V, b);
  } else {
    stv<BF16, V, false>(d_gate, e, n, a);
    stv<BF16, V, false>(d_up, e, n, b);
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------
bool dtype_ok(int32_t d) { return d == PRL_DTYPE_F32 || d == PRL_DTYPE_BF16; }

int check_shape(int64_t rows, int64_t cols) {
  PRL_CHECK_ARG(rows >= 0, "negative rows %lld", (long long)rows);
  PRL_CHECK_ARG(cols > 0, "cols %lld must be positive", (long long)cols);
  PRL_CHECK_ARG(cols < (int64_t(1) << 24), "cols %lld does not fit one launch", (long long)cols);
  int64_t numel = 0;
  PRL_CHECK_ARG(!__builtin_mul_overflow(rows, cols, &numel) && numel < (int64_t(1) << 46), "rows %lld x cols %lld elements are too many", (long long)rows,
                (long long)cols);
  PRL_CHECK_ARG(ceil_div(rows, kWaves) <= kMaxGrid, "rows %lld are too many for one launch", (long long)rows);
  return PRL_OK;
}

// the register-resident kernels: the smallest of 1, 2, 4, 8 wave iterations that covers the row; 0: the two-pass kernels
int row_iters(int64_t cols, int V, bool vec, int most = kMaxIters) {
  if (!vec) return 0;
  const int64_t n = ceil_div(cols, int64_t(kWave) * V);
  for (int it = 1; it <= most; it *= 2)
    if (n <= it) return it;
  return 0;
}

size_t workspace_need(int64_t rows, int64_t cols) { return size_t((ceil_div(rows, kBand) * cols * 4 + 15) & ~int64_t(15)); }

}  // namespace

extern "C" int prl_rmsnorm_workspace_bytes(int64_t rows, int64_t cols, size_t* bytes) {
  PRL_CHECK_ARG(bytes != nullptr, "bytes is null");
  if (int rc = check_shape(rows, cols)) return rc;
  *bytes = workspace_need(rows, cols);
  return PRL_OK;
}

extern "C" int prl_rmsnorm_fwd(int64_t rows, int64_t cols, const void* x, int32_t x_dtype, const void* weight, int32_t weight_dtype, float eps, void* out,
                               float* rstd, prl_stream_t stream) {
  if (int rc = check_shape(rows, cols)) return rc;
  PRL_CHECK_ARG(dtype_ok(x_dtype), "unknown x_dtype %d", x_dtype);
  PRL_CHECK_ARG(dtype_ok(weight_dtype), "unknown weight_dtype %d", weight_dtype);
  PRL_CHECK_ARG(eps >= 0.0f, "eps %g must not be negative", (double)eps);  // (a NaN fails too)
  if (rows == 0) return PRL_OK;
  PRL_CHECK_ARG(x != nullptr && weight != nullptr && out != nullptr && rstd != nullptr, "null pointer (x %p, weight %p, out %p, rstd %p)", x, weight, out,
                (void*)rstd);
  const bool xb = x_dtype == PRL_DTYPE_BF16, wb = weight_dtype == PRL_DTYPE_BF16;
  const int V = xb ? PRL_BODY_VEC_BF16 : PRL_BODY_VEC_F32;
  const bool vec = cols % V == 0 && prl::aligned16(x) && prl::aligned16(weight) && prl::aligned16(out);
  const int iters = row_iters(cols, V, vec);
  const dim3 grid(unsigned(ceil_div(rows, kWaves))), block(kBlock);
  hipStream_t st = static_cast<hipStream_t>(stream);
#define PRL_FWD_AS(XB, WB, VEC, ITERS) \
  hipLaunchKernelGGL((rmsnorm_fwd_kernel<XB, WB, VEC, ITERS>), grid, block, 0, st, x, weight, out, rstd, rows, int(cols), eps)
#define PRL_FWD(XB, WB)                                     \
  switch (iters) {                                          \
    case 1: PRL_FWD_AS(XB, WB, true, 1); break;             \
    case 2: PRL_FWD_AS(XB, WB, true, 2); break;             \
    case 4: PRL_FWD_AS(XB, WB, true, 4); break;             \
    case 8: PRL_FWD_AS(XB, WB, true, 8); break;             \
    default:                                                \
      if (vec) PRL_FWD_AS(XB, WB, true, 0);                 \
      else PRL_FWD_AS(XB, WB, false, 0);                    \
  }
  if (xb && wb) { PRL_FWD(true, true) }
  else if (xb) { PRL_FWD(true, false) }
  else if (wb) { PRL_FWD(false, true) }
  else { PRL_FWD(false, false) }
#undef PRL_FWD
#undef PRL_FWD_AS
  PRL_LAUNCH_CHECK("rmsnorm_fwd_kernel");
  return PRL_OK;
}

extern "C" int prl_rmsnorm_bwd(int64_t rows, int64_t cols, const void* x, int32_t x_dtype, const void* weight, int32_t weight_dtype, const float* rstd,
                               const void* grad_out, void* grad_x, float* grad_weight, void* workspace, size_t workspace_bytes, prl_stream_t stream) {
  if (int rc = check_shape(rows, cols)) return rc;
  PRL_CHECK_ARG(dtype_ok(x_dtype), "unknown x_dtype %d", x_dtype);
  PRL_CHECK_ARG(dtype_ok(weight_dtype), "unknown weight_dtype %d", weight_dtype);
  PRL_CHECK_ARG(grad_x != nullptr || grad_weight != nullptr, "neither grad_x nor grad_weight is wanted");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (rows == 0) {  // an empty sum: dw = 0
    if (grad_weight != nullptr) PRL_HIP_CHECK(hipMemsetAsync(grad_weight, 0, size_t(cols) * 4, st));
    return PRL_OK;
  }
  PRL_CHECK_ARG(x != nullptr && rstd != nullptr && grad_out != nullptr, "null pointer (x %p, rstd %p, grad_out %p)", x, (const void*)rstd, grad_out);
  PRL_CHECK_ARG(grad_x == nullptr || weight != nullptr, "null weight");
  const size_t need = workspace_need(rows, cols);
  if (grad_weight != nullptr) {
    PRL_CHECK_ARG(workspace != nullptr, "workspace is null");
    PRL_CHECK_ARG(prl::aligned16(workspace), "workspace is not 16-byte aligned");
    PRL_CHECK_ARG(workspace_bytes >= need, "workspace too small: %zu < %zu bytes", workspace_bytes, need);
  }
  const bool xb = x_dtype == PRL_DTYPE_BF16, wb = weight_dtype == PRL_DTYPE_BF16;
  const int V = xb ? PRL_BODY_VEC_BF16 : PRL_BODY_VEC_F32;
  // one path for both kinds of workgroup: 16-byte moves only when every array that is touched allows them
  const bool vec = cols % V == 0 && prl::aligned16(x) && prl::aligned16(grad_out) && (grad_x == nullptr || (prl::aligned16(weight) && prl::aligned16(grad_x)));
  // the backward keeps x AND g: 8 iterations of a bf16 row (with the weight's loads in flight) do not fit 128 registers
  const int iters = row_iters(cols, V, vec, xb ? 4 : kMaxIters);
  const int64_t dx_blocks = grad_x != nullptr ? ceil_div(rows, kWaves) : 0;
  const int64_t tiles = ceil_div(cols, int64_t(kWave) * V), bands = ceil_div(rows, kBand);
  const int64_t dw_blocks = grad_weight != nullptr ? tiles * bands : 0;
  PRL_CHECK_ARG(dx_blocks + dw_blocks <= kMaxGrid, "rows %lld x cols %lld are too many workgroups for one launch", (long long)rows, (long long)cols);
  float* partial = static_cast<float*>(workspace);
  const dim3 grid(unsigned(dx_blocks + dw_blocks)), block(kBlock);
#define PRL_BWD_AS(XB, WB, VEC, ITERS)                                                                                                        \
  hipLaunchKernelGGL((rmsnorm_bwd_kernel<XB, WB, VEC, ITERS>), grid, block, 0, st, x, weight, rstd, grad_out, grad_x, partial, rows, int(cols), \
                     int(dx_blocks), int(tiles))
#define PRL_BWD(XB, WB)                                     \
  switch (iters) {                                          \
    case 1: PRL_BWD_AS(XB, WB, true, 1); break;             \
    case 2: PRL_BWD_AS(XB, WB, true, 2); break;             \
    case 4: PRL_BWD_AS(XB, WB, true, 4); break;             \
    case 8: PRL_BWD_AS(XB, WB, true, (XB ? 4 : 8)); break;  \
    default:                                                \
      if (vec) PRL_BWD_AS(XB, WB, true, 0);                 \
      else PRL_BWD_AS(XB, WB, false, 0);                    \
  }
  if (xb && wb) { PRL_BWD(true, true) }
  else if (xb) { PRL_BWD(true, false) }
  else if (wb) { PRL_BWD(false, true) }
  else { PRL_BWD(false, false) }
#undef PRL_BWD
#undef PRL_BWD_AS
  PRL_LAUNCH_CHECK("rmsnorm_bwd_kernel");
  if (grad_weight != nullptr) {
    hipLaunchKernelGGL(rmsnorm_dw_fold_kernel, dim3(unsigned(ceil_div(cols, kBlock))), block, 0, st, partial, grad_weight, int(bands), int(cols));
    PRL_LAUNCH_CHECK("rmsnorm_dw_fold_kernel");
  }
  return PRL_OK;
}

namespace {

int check_flat(int64_t numel, int32_t dtype) {
  PRL_CHECK_ARG(numel >= 0, "negative numel %lld", (long long)numel);
  PRL_CHECK_ARG(dtype_ok(dtype), "unknown dtype %d", dtype);
  PRL_CHECK_ARG(ceil_div(numel, int64_t(kBlock) * kSwigluVec) <= kMaxGrid, "numel %lld is too large for one launch", (long long)numel);
  return PRL_OK;
}

}  // namespace

extern "C" int prl_swiglu_fwd(int64_t numel, const void* gate, const void* up, int32_t dtype, void* out, prl_stream_t stream) {
  if (int rc = check_flat(numel, dtype)) return rc;
  if (numel == 0) return PRL_OK;
  PRL_CHECK_ARG(gate != nullptr && up != nullptr && out != nullptr, "null pointer (gate %p, up %p, out %p)", gate, up, out);
  const bool aligned = prl::aligned16(gate) && prl::aligned16(up) && prl::aligned16(out);
  const dim3 grid(unsigned(ceil_div(numel, int64_t(kBlock) * kSwigluVec))), block(kBlock);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == PRL_DTYPE_BF16) {
    if (aligned) hipLaunchKernelGGL((swiglu_fwd_kernel<true, true>), grid, block, 0, st, gate, up, out, numel);
    else hipLaunchKernelGGL((swiglu_fwd_kernel<true, false>), grid, block, 0, st, gate, up, out, numel);
  } else {
    if (aligned) hipLaunchKernelGGL((swiglu_fwd_kernel<false, true>), grid, block, 0, st, gate, up, out, numel);
    else hipLaunchKernelGGL((swiglu_fwd_kernel<false, false>), grid, block, 0, st, gate, up, out, numel);
  }
  PRL_LAUNCH_CHECK("swiglu_fwd_kernel");
  return PRL_OK;
}

extern "C" int prl_swiglu_bwd(int64_t numel, const void* gate, const void* up, const void* grad_out, int32_t dtype, void* grad_gate, void* grad_up,
                              prl_stream_t stream) {
  if (int rc = check_flat(numel, dtype)) return rc;
  if (numel == 0) return PRL_OK;
  PRL_CHECK_ARG(gate != nullptr && up != nullptr && grad_out != nullptr && grad_gate != nullptr && grad_up != nullptr,
                "null pointer (gate %p, up %p, grad_out %p, grad_gate %p, grad_up %p)", gate, up, grad_out, grad_gate, grad_up);
  const bool aligned = prl::aligned16(gate) && prl::aligned16(up) && prl::aligned16(grad_out) && prl::aligned16(grad_gate) && prl::aligned16(grad_up);
  const dim3 grid(unsigned(ceil_div(numel, int64_t(kBlock) * kSwigluVec))), block(kBlock);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == PRL_DTYPE_BF16) {
    if (aligned) hipLaunchKernelGGL((swiglu_bwd_kernel<true, true>), grid, block, 0, st, gate, up, grad_out, grad_gate, grad_up, numel);
    else hipLaunchKernelGGL((swiglu_bwd_kernel<true, false>), grid, block, 0, st, gate, up, grad_out, grad_gate, grad_up, numel);
  } else {
    if (aligned) hipLaunchKernelGGL((swiglu_bwd_kernel<false, true>), grid, block, 0, st, gate, up, grad_out, grad_gate, grad_up, numel);
    else hipLaunchKernelGGL((swiglu_bwd_kernel<false, false>), grid, block, 0, st, gate, up, grad_out, grad_gate, grad_up, numel);
  }
  PRL_LAUNCH_CHECK("swiglu_bwd_kernel");
  return PRL_OK;
}
