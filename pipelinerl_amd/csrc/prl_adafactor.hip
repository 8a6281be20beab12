// Adafactor step of EVERY parameter as multi-tensor launches: transformers' Adafactor(relative_step=False, scale_parameter=False,
// beta1=None), which the reference's get_optimizer builds for "adafactor" (pipelinerl/finetune/optim.py:33-36), with the clip
// coefficient of prl_optim_grad_norm applied on the way in.  The arithmetic is prl_adafactor_math.h.
//
// A parameter is a batch of B matrices [R, C] (1-D: one run of elements, laid out as rows of 512).  One workgroup of 4 waves owns
// a band of kBand rows x a tile of kTile columns; a wave takes every fourth row of the band, a lane 8 columns of the tile: 8
// consecutive ones moved with 16-byte loads and stores where every row starts 16-byte aligned, else the columns lane, lane + 64, ...
// one element at a time (coalesced across the wave).  Per launch group (<= kSegs parameters, <= kGroupElems elements):
//   1. adafactor_stats_kernel   one read of the gradient: per row of a tile the fp64 sum of g^2 + eps1 over its columns, per
//                               column of a band the sum over its rows, as records in the workspace; 1-D: v is updated in place
//   2. adafactor_fold_kernel    a thread per row / per column folds its records in tile / band order, updates row / col, leaves
//                               rsqrt(col) in the workspace and the per-256-rows sums of the new row averages
//      adafactor_rowfac_kernel  a workgroup per matrix: mean of row in a fixed order, rsqrt(row / mean) into the workspace
//   3. adafactor_rms_kernel     second read of the gradient: per tile the fp64 sum of update^2
//      adafactor_denom_kernel   a workgroup per parameter folds its tiles in order: max(1, rms / clip_threshold)
//   4. adafactor_apply_kernel   third read of the gradient, read-modify-write of the fp32 weights (master copy or the parameter
//                               itself), round-to-nearest-even store of a bf16 parameter at its own address
// Algorithmic bytes per element, bf16 parameter + bf16 gradient + fp32 master: 2 + 2 + (2 + 4 read, 4 + 2 written) = 16; the
// records add 8 / kTile + 8 / kBand = 0.14.  No atomics; every sum has a fixed order, so two runs give the same bits.
#include "prl_common.h"
#include "prl_optim_io.h"
#include "prl_adafactor_math.h"

namespace {

using prl::kWave;
using namespace prl::optim_io;

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;
constexpr int kBand = 64;                        // rows per workgroup
constexpr int kTile = kWave * kGroup;            // 512 columns per workgroup
constexpr int kSegs = 32;                        // parameters per launch group: 32 x 104 B of kernel arguments
constexpr int64_t kGroupElems = int64_t(1) << 28;  // elements per launch group: bounds the workspace (records of one group at a time)
constexpr int64_t kMaxItems = int64_t(1) << 30;  // grids and prefix sums stay in int32

struct Seg {
  void* param;
  const void* grad;
  float* master;  // null: the parameter itself carries the weights
  float* v;       // unfactored only
  float* row;     // factored only: [B, R]
  float* col;     //                [B, C]
  int64_t ws;     // factored: byte offset of its region in the workspace
  int64_t numel;
  int32_t B, R, C;
  int32_t part0;  // index of its first tile among the group's sum-of-squares records
  PrlAdafactorScalars sc;
  uint8_t pb, gb, factored, vec;
};

struct Table {
  Seg seg[kSegs];
  int32_t first_tile[kSegs + 1];   // prefix sums: tiles (every segment)
  int32_t first_fold[kSegs + 1];   //              row + column fold items (factored segments)
  int32_t first_batch[kSegs + 1];  //              matrices (factored segments)
  int32_t n;
};

__host__ __device__ inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
__host__ __device__ inline int64_t align16(int64_t bytes) { return (bytes + 15) & ~int64_t(15); }

// a factored segment's part of the workspace
struct Region {
  float* rfac;      // [B, R]            rsqrt(row / mean(row))
  float* cfac;      // [B, C]            rsqrt(col)
  double* rowsum;   // [B, ceil(R/256)]  sums of the new row averages, 256 rows each
  double* rowpart;  // [tiles of C][B, R]   sum of g^2 + eps1 over the tile's columns
  double* colpart;  // [bands of R][B, C]   ... over the band's rows
  int64_t bytes;
};

__host__ __device__ inline Region region_of(char* base, int64_t B, int64_t R, int64_t C) {
  Region g;
  int64_t off = 0;
  g.rfac = reinterpret_cast<float*>(base + off);
  off += align16(B * R * 4);
  g.cfac = reinterpret_cast<float*>(base + off);
  off += align16(B * C * 4);
  g.rowsum = reinterpret_cast<double*>(base + off);
  off += align16(B * ceil_div(R, kBlock) * 8);
  g.rowpart = reinterpret_cast<double*>(base + off);
  off += align16(ceil_div(C, kTile) * B * R * 8);
  g.colpart = reinterpret_cast<double*>(base + off);
  off += align16(ceil_div(R, kBand) * B * C * 8);
  g.bytes = off;
  return g;
}

// the group's part in front of the regions: one fp64 record per tile, one fp32 denominator per segment
__host__ __device__ inline int64_t header_bytes(int64_t tiles) { return align16(tiles * 8) + align16(kSegs * 4); }
__device__ __forceinline__ double* tile_records(char* ws) { return reinterpret_cast<double*>(ws); }
__device__ __forceinline__ float* denominators(char* ws, int64_t tiles) { return reinterpret_cast<float*>(ws + align16(tiles * 8)); }

// ---- a lane's 8 slots of one row of a tile -----------------------------------------------------------------------------
// slot k is column c0 + k * cs: VEC: c0 = tile + 8 lane, cs = 1; else c0 = tile + lane, cs = 64.  `mask`: the slots inside the row.
template <bool VEC, bool BF16>
__device__ __forceinline__ void ld8(const void* base, int64_t e, int cs, unsigned mask, float (&o)[kGroup]) {
  if (VEC && mask == 0xffu) {
    load8<BF16>(base, e, o);
    return;
  }
#pragma unroll
  for (int k = 0; k < kGroup; ++k) o[k] = (mask >> k) & 1u ? load1<BF16>(base, e + int64_t(k) * cs) : 0.0f;
}

template <bool VEC, bool BF16, bool STREAM>
__device__ __forceinline__ void st8(void* base, int64_t e, int cs, unsigned mask, const float (&v)[kGroup]) {
  if (VEC && mask == 0xffu) {
    if constexpr (STREAM && !BF16) store8_stream(static_cast<float*>(base), e, v);
    else store8<BF16>(base, e, v);
    return;
  }
#pragma unroll
  for (int k = 0; k < kGroup; ++k)
    if ((mask >> k) & 1u) store1<BF16>(base, e + int64_t(k) * cs, v[k]);
}

struct TilePos {
  int b, r0, r1, tile0;  // matrix, rows [r0, r1) of it, first column of the tile
  int c0, cs;            // this lane's slot 0 and the slot stride
  unsigned cmask;        // slots with a column < C
};

template <bool VEC>
__device__ __forceinline__ TilePos tile_pos(const Seg& s, int t) {
  const int nct = int(ceil_div(s.C, kTile)), nrb = int(ceil_div(s.R, kBand));
  const int lane = threadIdx.x & (kWave - 1);
  TilePos p;
  p.b = t / (nrb * nct);
  const int rb = (t / nct) % nrb;
  p.tile0 = (t % nct) * kTile;
  p.r0 = rb * kBand;
  p.r1 = p.r0 + kBand < s.R ? p.r0 + kBand : s.R;
  p.c0 = p.tile0 + (VEC ? lane * kGroup : lane);
  p.cs = VEC ? 1 : kWave;
  p.cmask = 0;
#pragma unroll
  for (int k = 0; k < kGroup; ++k)
    if (p.c0 + k * p.cs < s.C) p.cmask |= 1u << k;
  return p;
}

// first element of row r of matrix b, and the slots of this lane that lie inside the parameter (the last row of a 1-D run is ragged)
__device__ __forceinline__ unsigned row_mask(const Seg& s, const TilePos& p, int r, int64_t& e) {
  e = (int64_t(p.b) * s.R + r) * s.C + p.c0;
  unsigned m = p.cmask;
  if (!s.factored) {
#pragma unroll
    for (int k = 0; k < kGroup; ++k)
      if (e + int64_t(k) * p.cs >= s.numel) m &= ~(1u << k);
  }
  return m;
}

// the four waves' values added in wave order; every thread gets the sum
__device__ __forceinline__ double block_sum(double v, double (&lds)[kWaves]) {
  v = prl::wave_sum(v);
  __syncthreads();  // (a previous use of lds is over)
  if ((threadIdx.x & (kWave - 1)) == 0) lds[threadIdx.x / kWave] = v;
  __syncthreads();
  double t = lds[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) t += lds[w];
  return t;
}

// ---- 1. row / column records of update = g^2 + eps1; 1-D: v -------------------------------------------------------------
template <bool VEC, bool GB>
__device__ __forceinline__ void stats_tile(const Seg& s, int t, float coef, double eps1, char* ws, double (&red)[kWaves][kTile]) {
  const TilePos p = tile_pos<VEC>(s, t);
  const int wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
  if (!s.factored) {
    for (int r = p.r0 + wave; r < p.r1; r += kWaves) {
      int64_t e;
      const unsigned m = row_mask(s, p, r, e);
      float g[kGroup], v[kGroup];
      ld8<VEC, GB>(s.grad, e, p.cs, m, g);
      ld8<VEC, false>(s.v, e, p.cs, m, v);
#pragma unroll
      for (int k = 0; k < kGroup; ++k) v[k] = prl_adafactor_average(s.sc, v[k], prl_adafactor_sq(prl_adafactor_grad(g[k], coef), eps1));
      st8<VEC, false, false>(s.v, e, p.cs, m, v);  // read again by the rms pass
    }
    return;
  }
  const Region reg = region_of(ws + s.ws, s.B, s.R, s.C);
  const int64_t rows = int64_t(s.B) * s.R, cols = int64_t(s.B) * s.C;
  double colacc[kGroup];
#pragma unroll
  for (int k = 0; k < kGroup; ++k) colacc[k] = 0.0;
  for (int r = p.r0 + wave; r < p.r1; r += kWaves) {
    int64_t e;
    const unsigned m = row_mask(s, p, r, e);
    float g[kGroup];
    ld8<VEC, GB>(s.grad, e, p.cs, m, g);
    double rs = 0.0;
#pragma unroll
    for (int k = 0; k < kGroup; ++k) {
      if ((m >> k) & 1u) {
        const double q = prl_adafactor_sq(prl_adafactor_grad(g[k], coef), eps1);
        colacc[k] += q;
        rs += q;
      }
    }
    rs = prl::wave_sum(rs);
    if (lane == 0) reg.rowpart[int64_t(p.tile0 / kTile) * rows + int64_t(p.b) * s.R + r] = rs;
  }
#pragma unroll
  for (int k = 0; k < kGroup; ++k) red[wave][(p.c0 - p.tile0) + k * p.cs] = colacc[k];
  __syncthreads();
  for (int j = threadIdx.x; j < kTile; j += kBlock) {
    const int c = p.tile0 + j;
    if (c < s.C) reg.colpart[int64_t(p.r0 / kBand) * cols + int64_t(p.b) * s.C + c] = ((red[0][j] + red[1][j]) + red[2][j]) + red[3][j];
  }
}

__global__ __launch_bounds__(kBlock) void adafactor_stats_kernel(const Table tab, const float* __restrict__ norm_and_coef, double eps1, char* __restrict__ ws) {
  __shared__ double red[kWaves][kTile];
  const int i = owner(tab.first_tile, tab.n, blockIdx.x);
  const Seg& s = tab.seg[i];
  const int t = blockIdx.x - tab.first_tile[i];
  const float coef = norm_and_coef ? norm_and_coef[1] : 1.0f;
  if (s.vec) {
    if (s.gb) stats_tile<true, true>(s, t, coef, eps1, ws, red);
    else stats_tile<true, false>(s, t, coef, eps1, ws, red);
  } else {
    if (s.gb) stats_tile<false, true>(s, t, coef, eps1, ws, red);
    else stats_tile<false, false>(s, t, coef, eps1, ws, red);
  }
}

// ---- 2. the records folded: row, col, rsqrt(col), sums of row ------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void adafactor_fold_kernel(const Table tab, char* __restrict__ ws) {
  __shared__ double lds[kWaves];
  const int i = owner(tab.first_fold, tab.n, blockIdx.x);
  const Seg& s = tab.seg[i];
  const int item = blockIdx.x - tab.first_fold[i];
  const Region reg = region_of(ws + s.ws, s.B, s.R, s.C);
  const int nrc = int(ceil_div(s.R, kBlock));
  const int64_t rows = int64_t(s.B) * s.R, cols = int64_t(s.B) * s.C;
  if (item < s.B * nrc) {  // 256 rows of one matrix
    const int b = item / nrc, r = (item % nrc) * kBlock + threadIdx.x;
    double mine = 0.0;
    if (r < s.R) {
      const int64_t at = int64_t(b) * s.R + r;
      const int nct = int(ceil_div(s.C, kTile));
      double t = 0.0;
      for (int ct = 0; ct < nct; ++ct) t += reg.rowpart[int64_t(ct) * rows + at];
      const float nw = prl_adafactor_average(s.sc, s.row[at], t / double(s.C));
      s.row[at] = nw;
      mine = double(nw);
    }
    const double tot = block_sum(mine, lds);
    if (threadIdx.x == 0) reg.rowsum[item] = tot;
  } else {  // 256 columns of the batch
    const int64_t j = int64_t(item - s.B * nrc) * kBlock + threadIdx.x;
    if (j < cols) {
      const int nrb = int(ceil_div(s.R, kBand));
      double t = 0.0;
      for (int rb = 0; rb < nrb; ++rb) t += reg.colpart[int64_t(rb) * cols + j];
      const float nw = prl_adafactor_average(s.sc, s.col[j], t / double(s.R));
      s.col[j] = nw;
      reg.cfac[j] = prl_adafactor_rsqrt(nw);
    }
  }
}

__global__ __launch_bounds__(kBlock) void adafactor_rowfac_kernel(const Table tab, char* __restrict__ ws) {
  __shared__ double lds[kWaves];
  const int i = owner(tab.first_batch, tab.n, blockIdx.x);
  const Seg& s = tab.seg[i];
  const int b = blockIdx.x - tab.first_batch[i];
  const Region reg = region_of(ws + s.ws, s.B, s.R, s.C);
  const int nrc = int(ceil_div(s.R, kBlock));
  double mine = 0.0;
  for (int k = threadIdx.x; k < nrc; k += kBlock) mine += reg.rowsum[int64_t(b) * nrc + k];
  const double mean = block_sum(mine, lds) / double(s.R);
  for (int r = threadIdx.x; r < s.R; r += kBlock) {
    const int64_t at = int64_t(b) * s.R + r;
    reg.rfac[at] = prl_adafactor_row_factor(s.row[at], mean);
  }
}

// ---- 3. / 4. update of one row's slots ------------------------------------------------------------------------------------
template <bool VEC, bool GB>
__device__ __forceinline__ void row_update(const Seg& s, const TilePos& p, const Region& reg, const float (&cf)[kGroup], int r, int64_t e, unsigned m,
                                           float coef, float (&u)[kGroup]) {
  float g[kGroup];
  ld8<VEC, GB>(s.grad, e, p.cs, m, g);
  if (s.factored) {
    const float rf = reg.rfac[int64_t(p.b) * s.R + r];
#pragma unroll
    for (int k = 0; k < kGroup; ++k) u[k] = prl_adafactor_update(rf, cf[k], prl_adafactor_grad(g[k], coef));
  } else {
    float v[kGroup];
    ld8<VEC, false>(s.v, e, p.cs, m, v);
#pragma unroll
    for (int k = 0; k < kGroup; ++k) u[k] = (m >> k) & 1u ? prl_adafactor_update(prl_adafactor_rsqrt(v[k]), 1.0f, prl_adafactor_grad(g[k], coef)) : 0.0f;
  }
}

__device__ __forceinline__ void column_factors(const Seg& s, const TilePos& p, const Region& reg, float (&cf)[kGroup]) {
#pragma unroll
  for (int k = 0; k < kGroup; ++k) cf[k] = s.factored && ((p.cmask >> k) & 1u) ? reg.cfac[int64_t(p.b) * s.C + p.c0 + k * p.cs] : 0.0f;
}

template <bool VEC, bool GB>
__device__ __forceinline__ double rms_tile(const Seg& s, int t, float coef, char* ws) {
  const TilePos p = tile_pos<VEC>(s, t);
  const int wave = threadIdx.x / kWave;
  const Region reg = region_of(ws + (s.factored ? s.ws : 0), s.B, s.R, s.C);  // (unfactored: never dereferenced)
  float cf[kGroup];
  column_factors(s, p, reg, cf);
  double acc = 0.0;
  for (int r = p.r0 + wave; r < p.r1; r += kWaves) {
    int64_t e;
    const unsigned m = row_mask(s, p, r, e);
    float u[kGroup];
    row_update<VEC, GB>(s, p, reg, cf, r, e, m, coef, u);
#pragma unroll
    for (int k = 0; k < kGroup; ++k)
      if ((m >> k) & 1u) acc += double(u[k]) * double(u[k]);
  }
  return acc;
}

__global__ __launch_bounds__(kBlock) void adafactor_rms_kernel(const Table tab, const float* __restrict__ norm_and_coef, char* __restrict__ ws) {
  __shared__ double lds[kWaves];
  const int i = owner(tab.first_tile, tab.n, blockIdx.x);
  const Seg& s = tab.seg[i];
  const int t = blockIdx.x - tab.first_tile[i];
  const float coef = norm_and_coef ? norm_and_coef[1] : 1.0f;
  double acc;
  if (s.vec) acc = s.gb ? rms_tile<true, true>(s, t, coef, ws) : rms_tile<true, false>(s, t, coef, ws);
  else acc = s.gb ? rms_tile<false, true>(s, t, coef, ws) : rms_tile<false, false>(s, t, coef, ws);
  acc = block_sum(acc, lds);
  if (threadIdx.x == 0) tile_records(ws)[s.part0 + t] = acc;
}

__global__ __launch_bounds__(kBlock) void adafactor_denom_kernel(const Table tab, double clip_threshold, char* __restrict__ ws) {
  __shared__ double lds[kWaves];
  const int i = blockIdx.x;
  const Seg& s = tab.seg[i];
  const int n = tab.first_tile[i + 1] - tab.first_tile[i];
  const double* rec = tile_records(ws) + s.part0;
  double mine = 0.0;
  for (int k = threadIdx.x; k < n; k += kBlock) mine += rec[k];
  const double tot = block_sum(mine, lds);
  if (threadIdx.x == 0) denominators(ws, tab.first_tile[tab.n])[i] = prl_adafactor_denom(tot, s.numel, clip_threshold);
}

// PB / GB: bf16 parameter / gradient; MW: fp32 master weights (the bf16 parameter is only written)
template <bool VEC, bool PB, bool GB, bool MW>
__device__ __forceinline__ void apply_tile(const Seg& s, int t, float coef, float denom, char* ws) {
  constexpr bool WB = MW ? false : PB;  // dtype of the array the weights are READ from
  const TilePos p = tile_pos<VEC>(s, t);
  const int wave = threadIdx.x / kWave;
  const Region reg = region_of(ws + (s.factored ? s.ws : 0), s.B, s.R, s.C);
  float cf[kGroup];
  column_factors(s, p, reg, cf);
  const void* w_src = MW ? static_cast<const void*>(s.master) : static_cast<const void*>(s.param);
  for (int r = p.r0 + wave; r < p.r1; r += kWaves) {
    int64_t e;
    const unsigned m = row_mask(s, p, r, e);
    float u[kGroup], w[kGroup];
    row_update<VEC, GB>(s, p, reg, cf, r, e, m, coef, u);
    ld8<VEC, WB>(w_src, e, p.cs, m, w);
#pragma unroll
    for (int k = 0; k < kGroup; ++k) w[k] = prl_adafactor_apply(s.sc, u[k], denom, w[k]);
    if constexpr (MW) st8<VEC, false, true>(s.master, e, p.cs, m, w);
    st8<VEC, PB, false>(s.param, e, p.cs, m, w);
  }
}

__global__ __launch_bounds__(kBlock) void adafactor_apply_kernel(const Table tab, const float* __restrict__ norm_and_coef, char* __restrict__ ws) {
  const int i = owner(tab.first_tile, tab.n, blockIdx.x);
  const Seg& s = tab.seg[i];
  const int t = blockIdx.x - tab.first_tile[i];
  const float coef = norm_and_coef ? norm_and_coef[1] : 1.0f;
  const float denom = denominators(ws, tab.first_tile[tab.n])[i];
  // wave-uniform dispatch on the segment's layout and dtypes (a master exists for bf16 parameters only)
#define PRL_APPLY(VEC)                                                                         \
  if (!s.pb) {                                                                                 \
    if (s.gb) apply_tile<VEC, false, true, false>(s, t, coef, denom, ws);                      \
    else apply_tile<VEC, false, false, false>(s, t, coef, denom, ws);                          \
  } else if (s.master) {                                                                       \
    if (s.gb) apply_tile<VEC, true, true, true>(s, t, coef, denom, ws);                        \
    else apply_tile<VEC, true, false, true>(s, t, coef, denom, ws);                            \
  } else {                                                                                     \
    if (s.gb) apply_tile<VEC, true, true, false>(s, t, coef, denom, ws);                       \
    else apply_tile<VEC, true, false, false>(s, t, coef, denom, ws);                           \
  }
  if (s.vec) { PRL_APPLY(true) } else { PRL_APPLY(false) }
#undef PRL_APPLY
}

// ---- host ---------------------------------------------------------------------------------------------------------------
bool live(const prl_adafactor_segment& s) { return s.grad != nullptr && s.batch > 0 && s.rows > 0 && s.cols > 0; }

int validate(const prl_adafactor_segment* segs, int64_t n) {
  PRL_CHECK_ARG(n >= 0, "negative segment count");
  PRL_CHECK_ARG(n == 0 || segs != nullptr, "null segment table with %lld segments", (long long)n);
  for (int64_t i = 0; i < n; ++i) {
    const prl_adafactor_segment& s = segs[i];
    PRL_CHECK_ARG(s.batch >= 0 && s.rows >= 0 && s.cols >= 0, "segment %lld: negative dimension (batch %lld, rows %lld, cols %lld)", (long long)i,
                  (long long)s.batch, (long long)s.rows, (long long)s.cols);
    int64_t numel = 0;
    PRL_CHECK_ARG(!__builtin_mul_overflow(s.batch, s.rows, &numel) && !__builtin_mul_overflow(numel, s.cols, &numel) && numel < (int64_t(1) << 40),
                  "segment %lld: batch %lld x rows %lld x cols %lld elements are too many for one launch", (long long)i, (long long)s.batch,
                  (long long)s.rows, (long long)s.cols);
    PRL_CHECK_ARG(s.grad_dtype == PRL_DTYPE_F32 || s.grad_dtype == PRL_DTYPE_BF16, "segment %lld: unknown grad_dtype %d", (long long)i, s.grad_dtype);
    PRL_CHECK_ARG(s.param_dtype == PRL_DTYPE_F32 || s.param_dtype == PRL_DTYPE_BF16, "segment %lld: unknown param_dtype %d", (long long)i, s.param_dtype);
    if (!live(s)) continue;
    PRL_CHECK_ARG(s.param != nullptr, "segment %lld: null param", (long long)i);
    if (s.v != nullptr) {
      PRL_CHECK_ARG(s.batch == 1 && s.rows == 1, "segment %lld: an unfactored segment (v is set) has batch = rows = 1, not %lld and %lld", (long long)i,
                    (long long)s.batch, (long long)s.rows);
    } else {
      PRL_CHECK_ARG(s.row != nullptr && s.col != nullptr, "segment %lld: a factored segment (v is null) needs row and col", (long long)i);
      PRL_CHECK_ARG(s.batch < (int64_t(1) << 31) && s.rows < (int64_t(1) << 31) && s.cols < (int64_t(1) << 31),
                    "segment %lld: a dimension of a factored segment does not fit 31 bits", (long long)i);
      PRL_CHECK_ARG(s.batch * ceil_div(s.rows, kBand) * ceil_div(s.cols, kTile) < kMaxItems && s.batch * ceil_div(s.rows, kBlock) + ceil_div(s.batch * s.cols, kBlock) < kMaxItems,
                    "segment %lld: batch %lld x rows %lld x cols %lld are too many tiles for one launch", (long long)i, (long long)s.batch, (long long)s.rows, (long long)s.cols);
    }
    PRL_CHECK_ARG(s.master == nullptr || s.param_dtype == PRL_DTYPE_BF16, "segment %lld: master weights go with a bf16 parameter", (long long)i);
    PRL_CHECK_ARG(s.step >= 1, "segment %lld: step %lld (the number of this update) must be >= 1", (long long)i, (long long)s.step);
  }
  return PRL_OK;
}

// The next launch group starting at segment `i`: fills `tab`, advances `i`, returns the bytes of workspace the group uses.
size_t next_group(const prl_adafactor_segment* segs, int64_t n, int64_t& i, double decay_rate, Table& tab) {
  tab.n = 0;
  tab.first_tile[0] = tab.first_fold[0] = tab.first_batch[0] = 0;
  int64_t tiles = 0, folds = 0, batches = 0, elems = 0, regions = 0;
  for (; i < n && tab.n < kSegs; ++i) {
    const prl_adafactor_segment& s = segs[i];
    if (!live(s)) continue;
    const bool factored = s.v == nullptr;
    const int64_t numel = s.batch * s.rows * s.cols;
    // a 1-D run of elements is laid out as rows of one tile's width: the last row is ragged
    const int64_t B = factored ? s.batch : 1, R = factored ? s.rows : ceil_div(numel, kTile), C = factored ? s.cols : kTile;
    const int64_t t = B * ceil_div(R, kBand) * ceil_div(C, kTile);
    const int64_t f = factored ? B * ceil_div(R, kBlock) + ceil_div(B * C, kBlock) : 0;
    if (tab.n > 0 && (elems + numel > kGroupElems || tiles + t >= kMaxItems || folds + f >= kMaxItems)) break;
    Seg& o = tab.seg[tab.n];
    o.param = s.param;
    o.grad = s.grad;
    o.master = static_cast<float*>(s.master);
    o.v = static_cast<float*>(s.v);
    o.row = static_cast<float*>(s.row);
    o.col = static_cast<float*>(s.col);
    o.ws = regions;  // (relative to the end of the group's header: fixed up below)
    o.numel = numel;
    o.B = int32_t(B), o.R = int32_t(R), o.C = int32_t(C);
    o.part0 = int32_t(tiles);
    o.sc = prl_adafactor_scalars(s.lr, s.weight_decay, decay_rate, s.step);
    o.pb = s.param_dtype == PRL_DTYPE_BF16, o.gb = s.grad_dtype == PRL_DTYPE_BF16, o.factored = factored;
    // 16-byte moves need every row of every array to start 16-byte aligned: 8 elements of bf16, 4 of fp32
    const bool rows_ok = C % ((o.pb || o.gb) ? 8 : 4) == 0;
    o.vec = rows_ok && prl::aligned16(s.param) && prl::aligned16(s.grad) && prl::aligned16(s.master) && prl::aligned16(s.v);
    if (factored) regions += region_of(nullptr, B, R, C).bytes;
    tiles += t, folds += f, batches += factored ? B : 0, elems += numel;
    ++tab.n;
    tab.first_tile[tab.n] = int32_t(tiles), tab.first_fold[tab.n] = int32_t(folds), tab.first_batch[tab.n] = int32_t(batches);
  }
  const int64_t head = header_bytes(tiles);
  for (int k = 0; k < tab.n; ++k) tab.seg[k].ws += head;
  return tab.n ? size_t(head + regions) : 0;
}

int check_rule(double eps1, double clip_threshold, double decay_rate) {
  PRL_CHECK_ARG(eps1 >= 0.0, "negative eps1 %g", eps1);
  PRL_CHECK_ARG(clip_threshold > 0.0, "clip_threshold %g must be positive", clip_threshold);
  PRL_CHECK_ARG(decay_rate <= 0.0, "decay_rate %g must not be positive (beta2t = 1 - step^decay_rate lies in [0, 1))", decay_rate);
  return PRL_OK;
}

}  // namespace

extern "C" int prl_adafactor_workspace_bytes(const prl_adafactor_segment* segments, int64_t n_segments, size_t* bytes) {
  PRL_CHECK_ARG(bytes != nullptr, "bytes is null");
  if (int rc = validate(segments, n_segments)) return rc;
  size_t need = 0;
  Table tab;
  for (int64_t i = 0; i < n_segments;) {
    const size_t g = next_group(segments, n_segments, i, -0.8, tab);
    need = g > need ? g : need;
  }
  *bytes = need;
  return PRL_OK;
}

extern "C" int prl_adafactor_step(const prl_adafactor_segment* segments, int64_t n_segments, double eps1, double clip_threshold, double decay_rate,
                                  const float* norm_and_coef, void* workspace, size_t workspace_bytes, prl_stream_t stream) {
  if (int rc = validate(segments, n_segments)) return rc;
  if (int rc = check_rule(eps1, clip_threshold, decay_rate)) return rc;
  Table tab;
  size_t need = 0;
  for (int64_t i = 0; i < n_segments;) {
    const size_t g = next_group(segments, n_segments, i, decay_rate, tab);
    need = g > need ? g : need;
  }
  if (need == 0) return PRL_OK;  // no segment has a gradient and elements
  PRL_CHECK_ARG(workspace != nullptr, "workspace is null");
  PRL_CHECK_ARG(prl::aligned16(workspace), "workspace is not 16-byte aligned");
  PRL_CHECK_ARG(workspace_bytes >= need, "workspace too small: %zu < %zu bytes", workspace_bytes, need);
  hipStream_t st = static_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(workspace);
  for (int64_t i = 0; i < n_segments;) {
    if (next_group(segments, n_segments, i, decay_rate, tab) == 0) break;  // only skipped segments were left
    const unsigned tiles = unsigned(tab.first_tile[tab.n]), folds = unsigned(tab.first_fold[tab.n]), batches = unsigned(tab.first_batch[tab.n]);
    hipLaunchKernelGGL(adafactor_stats_kernel, dim3(tiles), dim3(kBlock), 0, st, tab, norm_and_coef, eps1, ws);
    PRL_LAUNCH_CHECK("adafactor_stats_kernel");
    if (folds) {
      hipLaunchKernelGGL(adafactor_fold_kernel, dim3(folds), dim3(kBlock), 0, st, tab, ws);
      PRL_LAUNCH_CHECK("adafactor_fold_kernel");
      hipLaunchKernelGGL(adafactor_rowfac_kernel, dim3(batches), dim3(kBlock), 0, st, tab, ws);
      PRL_LAUNCH_CHECK("adafactor_rowfac_kernel");
    }
    hipLaunchKernelGGL(adafactor_rms_kernel, dim3(tiles), dim3(kBlock), 0, st, tab, norm_and_coef, ws);
    PRL_LAUNCH_CHECK("adafactor_rms_kernel");
    hipLaunchKernelGGL(adafactor_denom_kernel, dim3(unsigned(tab.n)), dim3(kBlock), 0, st, tab, clip_threshold, ws);
    PRL_LAUNCH_CHECK("adafactor_denom_kernel");
    hipLaunchKernelGGL(adafactor_apply_kernel, dim3(tiles), dim3(kBlock), 0, st, tab, norm_and_coef, ws);
    PRL_LAUNCH_CHECK("adafactor_apply_kernel");
  }
  return PRL_OK;
}

// tile geometry, for tests that place shapes at its edges: rows per band, columns per tile, segments and elements per launch group
extern "C" int prl_adafactor_geometry(int64_t* band_rows, int64_t* tile_cols, int64_t* group_segments, int64_t* group_elements) {
  PRL_CHECK_ARG(band_rows && tile_cols && group_segments && group_elements, "null output");
  *band_rows = kBand, *tile_cols = kTile, *group_segments = kSegs, *group_elements = kGroupElems;
  return PRL_OK;
}
