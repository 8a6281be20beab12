// Stochastic rounding of fp32 to bf16 for the compact optimizer state (prl_optim_compact.hip), and the counter-based generator
// that feeds it.  Compiles for host and device, like prl_optim_math.h; the host-compiled harness is
// tests/harness/optim_compact_host.cpp.
//
// Generator: Philox4x32 with 10 rounds (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): multipliers
// 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85.  A call is a pure function of (counter, key): no state lives
// anywhere, and a value depends on WHAT is rounded, never on which lane, chunk, piece or rank rounds it.
//
// One call serves the 4 consecutive elements 4q .. 4q+3 of a parameter:
//   counter = (q lo, q hi, step, parameter ordinal)      key = (seed lo, seed hi)
// with q = (the element's index INSIDE ITS PARAMETER) / 4, `step` the number of this update (low 32 bits) and `ordinal` the
// parameter's index in param_groups order.  Element 4q + j takes output word j = x and cuts three 16-bit values from it:
//   r_p = x & 0xffff   (the parameter)      r_m = x >> 16   (exp_avg)      r_v = r_p ^ r_m   (exp_avg_sq)
// each uniform on 0 .. 65535 and pairwise independent (any two of them determine x's halves one to one).
//
// sr(f, r): with u the bits of f, the result is (u + r) >> 16: the magnitude is rounded up with probability
// (u & 0xffff) / 65536 and down otherwise, so the expectation of the bf16 value is f.  NaN gives 0x7FC0 as
// prl_f32_to_bf16_rne does; +-inf and +-0 have zero low bits and cannot be crossed from below, so they are unchanged; a finite
// value above the largest bf16 may become inf, as it does under round-to-nearest.
#pragma once

#include "prl_optim_math.h"

struct PrlPhilox4 {
  uint32_t w[4];
};

PRL_OPT_HD uint32_t prl_mulhi_u32(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32); }

PRL_OPT_HD PrlPhilox4 prl_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int round = 0; round < 10; ++round) {
    const uint32_t hi0 = prl_mulhi_u32(M0, c0), lo0 = M0 * c0;
    const uint32_t hi1 = prl_mulhi_u32(M1, c2), lo1 = M1 * c2;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0;
    c1 = lo1;
    c2 = n2;
    c3 = lo0;
    k0 += W0;  // (the bump after the last round is unused)
    k1 += W1;
  }
  PrlPhilox4 o;
  o.w[0] = c0;
  o.w[1] = c1;
  o.w[2] = c2;
  o.w[3] = c3;
  return o;
}

// The call that serves the elements 4 group .. 4 group + 3 of parameter `ordinal` at update `step`.
PRL_OPT_HD PrlPhilox4 prl_sr_words(uint64_t group, uint32_t step, uint32_t ordinal, uint64_t seed) {
  return prl_philox4x32_10((uint32_t)group, (uint32_t)(group >> 32), step, ordinal, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// output word j of a call (selects, not an indexed array: on the device a runtime index would go through scratch memory)
PRL_OPT_HD uint32_t prl_sr_word(const PrlPhilox4& o, uint32_t j) { return j == 0 ? o.w[0] : j == 1 ? o.w[1] : j == 2 ? o.w[2] : o.w[3]; }

PRL_OPT_HD uint32_t prl_sr_rp(uint32_t x) { return x & 0xffffu; }
PRL_OPT_HD uint32_t prl_sr_rm(uint32_t x) { return x >> 16; }
PRL_OPT_HD uint32_t prl_sr_rv(uint32_t x) { return (x & 0xffffu) ^ (x >> 16); }

// r in 0 .. 65535
PRL_OPT_HD uint16_t prl_f32_to_bf16_sr(float f, uint32_t r) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0;
  return (uint16_t)((u + r) >> 16);  // no carry out of 32 bits: the largest non-NaN pattern is 0xff800000
}
