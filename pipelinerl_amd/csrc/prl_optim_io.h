// Register <-> memory moves shared by the optimizer kernels (prl_optim.hip, prl_adafactor.hip): 8 consecutive elements of an
// fp32 / bf16 array with 16-byte loads and stores, their one-element forms for unaligned views and tails, and the scalar binary
// search that maps a workgroup to the segment that owns it.
#pragma once

#include "prl_common.h"
#include "prl_optim_math.h"

namespace prl {
namespace optim_io {

constexpr int kGroup = 8;  // elements per lane and iteration

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- 8 consecutive elements of an fp32 / bf16 array <-> registers -------------------------------------------------
template <bool BF16>
__device__ __forceinline__ void load8(const void* base, int64_t i, float (&o)[kGroup]) {
  if constexpr (BF16) {
    const u32x4 t = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(static_cast<const uint16_t*>(base) + i));
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      o[2 * k] = __uint_as_float(t[k] << 16);
      o[2 * k + 1] = __uint_as_float(t[k] & 0xffff0000u);
    }
  } else {
    const f32x4* p = reinterpret_cast<const f32x4*>(static_cast<const float*>(base) + i);
    const f32x4 a = __builtin_nontemporal_load(p);
    const f32x4 b = __builtin_nontemporal_load(p + 1);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      o[k] = a[k];
      o[4 + k] = b[k];
    }
  }
}

template <bool BF16>
__device__ __forceinline__ void store8(void* base, int64_t i, const float (&v)[kGroup]) {
  if constexpr (BF16) {
    u32x4 t;
#pragma unroll
    for (int k = 0; k < 4; ++k) t[k] = (uint32_t)prl_f32_to_bf16_rne(v[2 * k]) | ((uint32_t)prl_f32_to_bf16_rne(v[2 * k + 1]) << 16);
    *reinterpret_cast<u32x4*>(static_cast<uint16_t*>(base) + i) = t;  // the parameter is read again by the next forward: a plain store
  } else {
    f32x4* p = reinterpret_cast<f32x4*>(static_cast<float*>(base) + i);
    p[0] = f32x4{v[0], v[1], v[2], v[3]};
    p[1] = f32x4{v[4], v[5], v[6], v[7]};
  }
}

__device__ __forceinline__ void store8_stream(float* base, int64_t i, const float (&v)[kGroup]) {  // optimizer state: touched once per step
  f32x4* p = reinterpret_cast<f32x4*>(base + i);
  __builtin_nontemporal_store(f32x4{v[0], v[1], v[2], v[3]}, p);
  __builtin_nontemporal_store(f32x4{v[4], v[5], v[6], v[7]}, p + 1);
}

template <bool BF16>
__device__ __forceinline__ float load1(const void* base, int64_t i) {
  if constexpr (BF16) return prl_bf16_to_f32(static_cast<const uint16_t*>(base)[i]);
  else return static_cast<const float*>(base)[i];
}

template <bool BF16>
__device__ __forceinline__ void store1(void* base, int64_t i, float v) {
  if constexpr (BF16) static_cast<uint16_t*>(base)[i] = prl_f32_to_bf16_rne(v);
  else static_cast<float*>(base)[i] = v;
}

__device__ __forceinline__ bool aligned16_dev(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// which segment owns work item `c` (first = prefix sums of the segments' item counts)
template <int N>
__device__ __forceinline__ int owner(const int32_t (&first)[N], int n, int c) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (first[mid] <= c) lo = mid; else hi = mid;
  }
  return lo;
}

}  // namespace optim_io
}  // namespace prl
